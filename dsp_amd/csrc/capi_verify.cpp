// capi_verify.cpp -- the C ABI of float speaker verification (include/dsp_amd.h dsp_speaker_verif*, dsp_speaker_float_scan_device;
// DESIGN.md 3.13, 3.16): argument checks, all of them before a device is touched, the verifier's UBM (a GmmModel of gmm_model.hpp,
// uploaded by the first call that scores), its grow-only workspace (the per-clip entry's tile partials, the scan's per-row ll), the split
// of a large call over runs of clips or of windows, and the launches of verify_kernels.hip.
#include <cmath>
#include <cstdlib>
#include <memory>

#include "capi_util.hpp"
#include "verify_kernels.hpp"

using dsp::capi_fail;

struct dsp_speaker_verifier : dsp::Handle {
    int k = 0, d = 0;
    std::vector<float> host;             // log_consts[k], means[k][d], inv_covs[k][d], rounded once to float32
    dsp::DeviceBuf<float> model;         // the same on the device, from the first call that scores
    dsp::DeviceBuf<double> partials;     // grow-only: [chunks of a run of clips][4 tiles][1 + S]; the scan's float ll [1 + S][rows of a run]
    size_t max_run_doubles = 0;          // what the partials of one run of clips may take before a call is split
    size_t max_run_floats = 0;           // what the ll of one run of windows may take before a scan is split
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

// the same bound for the scan's ll of one run of windows (one window is never cut): 256 MiB, or DSP_AMD_VERIFY_SCAN_RUN_FLOATS floats
constexpr size_t kMaxRunFloats = (size_t)1 << 26;

size_t max_run_floats()
{
    const char *e = std::getenv("DSP_AMD_VERIFY_SCAN_RUN_FLOATS");
    const long long n = e ? std::atoll(e) : 0;
    return n > 0 ? (size_t)n : kMaxRunFloats;
}

// the UBM on the verifier's device (current), from the first call that scores
int upload_ubm(dsp_speaker_verifier *v) { return v->model.get() ? DSP_OK : dsp::upload_ubm(v->host, v->model); }

// one run of consecutive windows of a scan: pieces [p0, p1) of the plan, scored into ll[1 + S][pitch] from row `base` of the matrix
struct ScanRun {
    size_t p0, p1;
    long base, pitch, chunks, windows, window0;      // window0: the run's first window in the call's numbering
};

// The plan of a scan.  Window j of a recording of R rows at f is rows [f + j hop, f + j hop + n), n = min(win, R).  A run takes consecutive
// windows while the rows from its first window's first row (base) to its last window's end fit max_rows, and at least one window; what
// it takes of one recording is a piece (verify_kernels.hpp).  Rows shared by the windows of two runs are scored in both.  false: a run
// of more chunks or windows than a grid holds.
struct ScanPlan {
    std::vector<dsp::RowSpan> pieces, wins;
    std::vector<ScanRun> runs;
    long most = 0;                                   // the largest pitch
};

bool plan_scan(const long *frame_offsets, long n_recordings, long win, long hop, long max_rows, ScanPlan &plan)
{
    ScanRun run{0, 0, 0, 0, 0, 0, 0};
    long total = 0;
    auto close = [&] {
        run.p1 = plan.pieces.size();
        plan.runs.push_back(run);
        plan.most = std::max(plan.most, run.pitch);
        total += run.windows;
        run = ScanRun{plan.pieces.size(), 0, 0, 0, 0, 0, total};
    };
    for (long r = 0; r < n_recordings; ++r) {
        const long f = frame_offsets[r], R = frame_offsets[r + 1] - f;
        const long n = std::min(win, R), W = R >= win ? 1 + (R - win) / hop : 1;
        for (long j = 0; j < W;) {
            if (run.windows == 0) run.base = f + j * hop;
            const long room = run.base + max_rows - n - f;          // the last window that fits starts at or before f + room
            long j1 = room >= 0 ? std::min(W - 1, room / hop) : -1;
            if (j1 < j) {
                if (run.windows > 0) { close(); continue; }         // the next run starts at this window
                j1 = j;                                              // a run of its own for a window that fits none
            }
            const long rows = (j1 - j) * hop + n;
            plan.pieces.push_back(dsp::RowSpan{f + j * hop, run.chunks, rows});
            plan.wins.push_back(dsp::RowSpan{f + j * hop, run.windows, n});
            run.chunks += (rows + dsp::kVerifyChunkRows - 1) / dsp::kVerifyChunkRows;
            run.windows += j1 - j + 1;
            run.pitch = f + j * hop + rows - run.base;
            j = j1 + 1;
            if (run.chunks > INT32_MAX || run.windows > INT32_MAX) return false;
        }
    }
    if (run.windows > 0) close();
    return true;
}

}  // namespace

extern "C" {

int dsp_speaker_verifier_create(const dsp_gmm_float_params *ubm, int device, dsp_speaker_verifier **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (const int rc = dsp::check_gmm_float_params(ubm, "ubm", "ubm: ")) return rc;
    // no device is touched here: the UBM goes up in the first call that scores, which is also where a device that does not exist is reported
    return dsp::create_on_host(device, out, [&](dsp_speaker_verifier &v) -> int {
        if (const int rc = dsp::pack_ubm(ubm, v.host)) return rc;
        v.max_run_doubles = max_run_doubles();
        v.max_run_floats = max_run_floats();
        v.k = ubm->k;
        v.d = ubm->d;
        return DSP_OK;
    });
}

void dsp_speaker_verifier_destroy(dsp_speaker_verifier *v) { dsp::destroy(v); }

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
    if (const int rc = upload_ubm(v)) return rc;
    // runs of consecutive clips whose partials fit max_run_doubles (at least one clip each); a clip's unit0 counts chunks within its run
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(v->spans, (size_t)n_clips * sizeof(dsp::RowSpan), slot)) return rc;
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

int dsp_speaker_float_scan_device(dsp_speaker_verifier *v, const float *d_feats, long n_recordings, const long *frame_offsets, const dsp_scan_config *cfg,
                                  const float *d_means, long n_speakers, float *d_llr, float *d_ll_ubm, float *d_ll_target, int *d_best, float *d_best_llr,
                                  void *stream)
{
    if (!v) return capi_fail(DSP_EINVAL, "verifier is NULL");
    if (n_recordings < 0 || n_speakers < 0) return capi_fail(DSP_EINVAL, "n_recordings and n_speakers must be >= 0");
    if (n_recordings == 0 || n_speakers == 0) return DSP_OK;
    if (const int rc = dsp::scan_args(cfg, n_recordings)) return rc;
    if (!d_llr && !d_ll_ubm && !d_ll_target && !d_best && !d_best_llr) return capi_fail(DSP_EINVAL, "every output is NULL");
    if (n_recordings > kMaxClips) return capi_fail(DSP_EINVAL, "at most 2^30 recordings per call");
    if (n_speakers > dsp::kVerifyMaxSpeakers) return capi_fail(DSP_EINVAL, "at most 2^19 speakers per call");
    if (!d_feats) return capi_fail(DSP_EINVAL, "d_feats is NULL");
    if (!d_means) return capi_fail(DSP_EINVAL, "d_means is NULL");
    if (!frame_offsets) return capi_fail(DSP_EINVAL, "frame_offsets is NULL");
    if (const int rc = dsp::check_frame_offsets(frame_offsets, n_recordings)) return rc;
    if (const int rc = dsp::refuse_rowless(frame_offsets, n_recordings, " has no rows (the scores are means over a window's rows)")) return rc;
    ScanPlan plan;
    const long max_rows = (long)std::min<size_t>(v->max_run_floats / (size_t)(n_speakers + 1), (size_t)1 << 40);
    if (!plan_scan(frame_offsets, n_recordings, cfg->window_frames, cfg->hop_frames, max_rows, plan))
        return capi_fail(DSP_EINVAL, "2^31 windows or 2^39 rows, or more, in one run of windows");
    if (const int rc = dsp::check_device(v->device)) return rc;
    DSP_ON_DEVICE(v->device);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = upload_ubm(v)) return rc;
    if (v->partials.reserve(dsp::verify_scan_floats(plan.most, n_speakers) * sizeof(float)) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc of the verifier's workspace");
    const size_t P = plan.pieces.size(), bytes = P * sizeof(dsp::RowSpan);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(v->spans, 2 * bytes, slot)) return rc;
    std::memcpy(slot.h(), plan.pieces.data(), bytes);
    std::memcpy(static_cast<char *>(slot.h()) + bytes, plan.wins.data(), bytes);
    DSP_CAPI_HIP(slot.upload(2 * bytes, st));
    const dsp::RowSpan *d_pieces = static_cast<const dsp::RowSpan *>(slot.d()), *d_wins = d_pieces + P;
    float *ws = reinterpret_cast<float *>(v->partials.get());
    const size_t S = (size_t)n_speakers;
    for (const ScanRun &q : plan.runs) {
        const size_t w0 = (size_t)q.window0;
        DSP_CAPI_HIP(dsp::launch_verify_scan(d_feats, d_pieces + q.p0, d_wins + q.p0, (long)(q.p1 - q.p0), q.chunks, q.windows, cfg->window_frames, cfg->hop_frames,
                                             q.base, q.pitch, dsp::GmmModel{v->model, v->k, v->d}, d_means, n_speakers, ws, d_llr ? d_llr + w0 * S : nullptr,
                                             d_ll_ubm ? d_ll_ubm + w0 : nullptr, d_ll_target ? d_ll_target + w0 * S : nullptr, d_best ? d_best + w0 : nullptr,
                                             d_best_llr ? d_best_llr + w0 : nullptr, st));
    }
    return DSP_OK;
}

}  // extern "C"
