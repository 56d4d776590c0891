// capi_verify.cpp -- the C ABI of float speaker verification (include/dsp_amd.h dsp_speaker_verif*): argument checks, all
// of them before a device is touched, the verifier's UBM (a GmmModel of gmm_model.hpp, uploaded by the first call that scores), its
// grow-only workspace of tile partials, the split of a large call over runs of clips, and the launches of verify_kernels.hip.
#include <cmath>
#include <cstdlib>
#include <memory>

#include "capi_util.hpp"
#include "verify_kernels.hpp"

using dsp::capi_fail;

struct dsp_speaker_verifier {
    int device = 0, k = 0, d = 0;
    std::vector<float> host;             // log_consts[k], means[k][d], inv_covs[k][d], rounded once to float32
    dsp::DeviceBuf<float> model;         // the same on the device, from the first call that scores
    dsp::DeviceBuf<double> partials;     // grow-only: [chunks of a run of clips][4 tiles][1 + S]
    size_t max_run_doubles = 0;          // what the partials of one run of clips may take before a call is split
    dsp::SpanRing spans;
};

namespace {

// what the partials of one run of clips may take before a call is split (one clip is never split: its partials are what they are):
// 256 MiB, or DSP_AMD_VERIFY_RUN_DOUBLES doubles (read at create: how the tests reach the split with small batches)
constexpr size_t kMaxRunDoubles = (size_t)1 << 25;

size_t max_run_doubles()
{
    const char *e = std::getenv("DSP_AMD_VERIFY_RUN_DOUBLES");
    const long long n = e ? std::atoll(e) : 0;
    return n > 0 ? (size_t)n : kMaxRunDoubles;
}
constexpr long kMaxClips = 1L << 30;

}  // namespace

extern "C" {

int dsp_speaker_verifier_create(const dsp_gmm_float_params *ubm, int device, dsp_speaker_verifier **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (const int rc = dsp::check_gmm_float_params(ubm, "ubm", "ubm: ")) return rc;
    if (device < 0) return capi_fail(DSP_EINVAL, "device index out of range");
    auto v = std::make_unique<dsp_speaker_verifier>();
    v->host = dsp::pack_gmm_model(ubm->k, ubm->d, ubm->log_consts, ubm->means, ubm->inv_covs);
    for (const float x : v->host)
        if (!std::isfinite(x)) return capi_fail(DSP_EINVAL, "ubm: log_consts, means and inv_covs must be finite in float32");
    // no device is touched here: the UBM goes up in the first call that scores, which is also where a device that does not exist is reported
    v->device = device;
    v->max_run_doubles = max_run_doubles();
    v->k = ubm->k;
    v->d = ubm->d;
    *out = v.release();
    return DSP_OK;
}

void dsp_speaker_verifier_destroy(dsp_speaker_verifier *v)
{
    if (!v) return;
    dsp::DeviceScope scope(v->device);
    v->spans.release();
    delete v;
}

int dsp_speaker_verify_ragged_device(dsp_speaker_verifier *v, const float *d_feats, long n_clips, const long *frame_offsets, const float *d_means,
                                     long n_speakers, float *d_llr, float *d_ll_ubm, float *d_ll_target, int *d_best, float *d_best_llr, void *stream)
{
    if (!v) return capi_fail(DSP_EINVAL, "verifier is NULL");
    if (n_clips < 0 || n_speakers < 0) return capi_fail(DSP_EINVAL, "n_clips and n_speakers must be >= 0");
    if (n_clips == 0 || n_speakers == 0) return DSP_OK;
    if (!d_llr && !d_ll_ubm && !d_ll_target && !d_best && !d_best_llr) return capi_fail(DSP_EINVAL, "every output is NULL");
    if (n_clips > kMaxClips) return capi_fail(DSP_EINVAL, "at most 2^30 clips per call");
    if (n_speakers > dsp::kVerifyMaxSpeakers) return capi_fail(DSP_EINVAL, "at most 2^19 speakers per call");
    if (!d_feats) return capi_fail(DSP_EINVAL, "d_feats is NULL");
    if (!d_means) return capi_fail(DSP_EINVAL, "d_means is NULL");
    if (!frame_offsets) return capi_fail(DSP_EINVAL, "frame_offsets is NULL");
    if (const int rc = dsp::check_frame_offsets(frame_offsets, n_clips, "clip")) return rc;
    if (const int rc = dsp::refuse_rowless(frame_offsets, n_clips, " has no rows", "clip")) return rc;
    if (const int rc = dsp::check_device(v->device)) return rc;
    DSP_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    if (!v->model.get()) {
        if (v->model.alloc(v->host.size() * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the UBM");
        const hipError_t e = hipMemcpy(v->model, v->host.data(), v->host.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            v->model.reset();
            return capi_fail(DSP_EHIP, std::string("hipMemcpy of the UBM: ") + hipGetErrorString(e));
        }
    }
    // runs of consecutive clips whose partials fit max_run_doubles (at least one clip each); a clip's unit0 counts chunks within its run
    dsp::SpanRing::Lease slot;
    const hipError_t e = v->spans.acquire((size_t)n_clips * sizeof(dsp::RowSpan), slot);
    if (e != hipSuccess) return capi_fail(DSP_EHIP, std::string("the span ring: ") + hipGetErrorString(e));
    dsp::RowSpan *h = static_cast<dsp::RowSpan *>(slot.h());
    const size_t per_chunk = dsp::verify_partial_doubles(1, n_speakers);
    std::vector<long> run_start{0};
    long chunks = 0, most = 0;
    for (long c = 0; c < n_clips; ++c) {
        const long rows = frame_offsets[c + 1] - frame_offsets[c];
        const long mine = (rows + dsp::kVerifyChunkRows - 1) / dsp::kVerifyChunkRows;
        if (chunks > 0 && (size_t)(chunks + mine) * per_chunk > v->max_run_doubles) {
            run_start.push_back(c);
            chunks = 0;
        }
        h[c] = dsp::RowSpan{frame_offsets[c], chunks, rows};
        chunks += mine;
        most = std::max(most, chunks);
    }
    run_start.push_back(n_clips);
    if (most > INT32_MAX) return capi_fail(DSP_EINVAL, "a clip of 2^39 rows or more");
    if (v->partials.reserve(dsp::verify_partial_doubles(most, n_speakers) * sizeof(double)) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc of the verifier's workspace");
    DSP_CAPI_HIP(slot.upload((size_t)n_clips * sizeof(dsp::RowSpan), st));
    const dsp::RowSpan *d_spans = static_cast<const dsp::RowSpan *>(slot.d());
    const size_t S = (size_t)n_speakers;
    for (size_t r = 0; r + 1 < run_start.size(); ++r) {
        const long c0 = run_start[r], c1 = run_start[r + 1];
        const long rows_last = h[c1 - 1].n, run_chunks = h[c1 - 1].unit0 + (rows_last + dsp::kVerifyChunkRows - 1) / dsp::kVerifyChunkRows;
        DSP_CAPI_HIP(dsp::launch_verify(d_feats, d_spans + c0, c1 - c0, run_chunks, dsp::GmmModel{v->model, v->k, v->d}, d_means, n_speakers, v->partials,
                                        d_llr ? d_llr + (size_t)c0 * S : nullptr, d_ll_ubm ? d_ll_ubm + c0 : nullptr,
                                        d_ll_target ? d_ll_target + (size_t)c0 * S : nullptr, d_best ? d_best + c0 : nullptr,
                                        d_best_llr ? d_best_llr + c0 : nullptr, st));
    }
    return DSP_OK;
}

}  // extern "C"
