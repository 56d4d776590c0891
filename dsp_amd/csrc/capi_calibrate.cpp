// capi_calibrate.cpp -- the C ABI of score calibration (include/dsp_amd.h dsp_calibration_*): argument checks, all of them
// before a device is touched and in the order the header states, the host-only duration term, the calibrator's grow-only workspace
// and the labels and duration terms that travel through its ring to the kernels of calibrate_kernels.hip.
#include <cmath>

#include "calibrate_kernels.hpp"
#include "capi_util.hpp"

using dsp::capi_fail;

static_assert(sizeof(dsp_calibration) == 24, "dsp_calibration is 24 bytes (dsp_amd/lib.py Calibration)");
static_assert(sizeof(dsp_calibration_config) == 24, "dsp_calibration_config is 24 bytes (dsp_amd/lib.py CalibrationConfig)");
static_assert(sizeof(dsp_calibration_report) == 88, "dsp_calibration_report is 88 bytes (dsp_amd/lib.py CalibrationReport)");
static_assert(sizeof(dsp::CalState) <= 256, "the state lies in the first 256 bytes of the workspace");

struct dsp_calibrator : dsp::StageHandle {};      // ws: CalState, then the partials of every level (calibrate_kernels.hpp); spans: duration terms | truth

namespace {

double duration_term(long n_frames) { return std::log((double)n_frames + 1e-8); }

int check_frames(const long *n_frames, long n_rows)
{
    for (long r = 0; r < n_rows; ++r)
        if (n_frames[r] < 0) return capi_fail(DSP_EINVAL, "n_frames[" + std::to_string(r) + "] = " + std::to_string(n_frames[r]) + " is negative");
    return DSP_OK;
}

bool finite(const dsp_calibration &p) { return std::isfinite(p.a) && std::isfinite(p.b) && std::isfinite(p.c); }

}  // namespace

extern "C" {

int dsp_calibrator_create(int device, dsp_calibrator **out) { return dsp::create_on_host(device, out); }

void dsp_calibrator_destroy(dsp_calibrator *c) { dsp::destroy(c); }

int dsp_calibration_duration_term(const long *n_frames, long n_rows, double *out)
{
    if (n_rows < 0) return capi_fail(DSP_EINVAL, "n_rows < 0");
    if (n_rows == 0) return DSP_OK;
    if (!n_frames || !out) return capi_fail(DSP_EINVAL, "n_frames and out must not be NULL");
    if (const int rc = check_frames(n_frames, n_rows)) return rc;
    for (long r = 0; r < n_rows; ++r) out[r] = duration_term(n_frames[r]);
    return DSP_OK;
}

int dsp_calibration_fit_device(dsp_calibrator *c, const float *d_scores, long n_rows, long n_columns, const int *truth, const long *n_frames,
                               const dsp_calibration_config *cfg, const dsp_calibration *init, dsp_calibration_report *report, void *stream)
{
    if (!c) return capi_fail(DSP_EINVAL, "calibrator is NULL");
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_calibration_config is NULL");
    if (!(cfg->prior > 0.0 && cfg->prior < 1.0)) return capi_fail(DSP_EINVAL, "dsp_calibration_config: prior must lie inside (0, 1)");
    if (!(cfg->tol > 0.0)) return capi_fail(DSP_EINVAL, "dsp_calibration_config: tol must be > 0");
    if (cfg->max_iter < 1 || cfg->max_iter > dsp::kCalMaxIter)
        return capi_fail(DSP_EINVAL, "dsp_calibration_config: max_iter must be 1 .. 10000, got " + std::to_string(cfg->max_iter));
    if (!report) return capi_fail(DSP_EINVAL, "report is NULL");
    if (const int rc = dsp::check_score_shape(n_rows, n_columns)) return rc;
    const dsp_calibration start = init ? *init : dsp_calibration{1.0, 0.0, 0.0};
    if (!finite(start)) return capi_fail(DSP_EINVAL, "init is not finite");
    if (start.c != 0.0 && !n_frames) return capi_fail(DSP_EINVAL, "init->c != 0 without n_frames");
    if (n_rows == 0) {
        *report = dsp_calibration_report{start, 0, 0, 0, NAN, NAN, NAN, 0, 0, DSP_CAL_NO_CLASS, 0};
        return DSP_OK;
    }
    if (!d_scores) return capi_fail(DSP_EINVAL, "d_scores is NULL");
    if (!truth) return capi_fail(DSP_EINVAL, "truth is NULL");
    if (const int rc = dsp::check_truth(truth, n_rows, n_columns)) return rc;
    if (n_frames)
        if (const int rc = check_frames(n_frames, n_rows)) return rc;
    if (const int rc = dsp::check_trial_count(n_rows, n_columns)) return rc;
    if (const int rc = dsp::check_device(c->device)) return rc;
    DSP_ON_DEVICE(c->device);
    hipStream_t st = (hipStream_t)stream;
    // duration terms, T doubles (with n_frames) | truth, T ints
    const size_t n = (size_t)n_rows, bytes = (n_frames ? n * sizeof(double) : 0) + n * sizeof(int);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(c->spans, bytes, slot)) return rc;
    double *h_duration = static_cast<double *>(slot.h());
    int *h_truth = reinterpret_cast<int *>(h_duration + (n_frames ? n : 0));
    if (n_frames)
        for (long r = 0; r < n_rows; ++r) h_duration[r] = duration_term(n_frames[r]);
    std::memcpy(h_truth, truth, n * sizeof(int));
    if (c->ws.reserve(dsp::cal_workspace_bytes(n_rows, n_columns)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the calibrator's workspace");
    DSP_CAPI_HIP(slot.upload(bytes, st));
    const double *d_duration = static_cast<const double *>(slot.d());
    dsp::CalFit fit{d_scores, reinterpret_cast<const int *>(d_duration + (n_frames ? n : 0)), n_frames ? d_duration : nullptr, n_rows, n_columns, cfg->prior, cfg->tol,
                    cfg->max_iter, start, reinterpret_cast<dsp::CalState *>(c->ws.get()), reinterpret_cast<dsp::CalPartial *>(c->ws.get() + 256)};
    DSP_CAPI_HIP(dsp::launch_calibration_fit(fit, st));
    DSP_CAPI_HIP(hipMemcpyAsync(report, &fit.state->report, sizeof(*report), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    return DSP_OK;
}

int dsp_calibration_apply_device(dsp_calibrator *c, const float *d_scores, long n_rows, long n_columns, const long *n_frames, const dsp_calibration *params,
                                 float *d_out, void *stream)
{
    if (!c) return capi_fail(DSP_EINVAL, "calibrator is NULL");
    if (!params) return capi_fail(DSP_EINVAL, "params is NULL");
    if (!finite(*params)) return capi_fail(DSP_EINVAL, "params are not finite");
    if (const int rc = dsp::check_score_shape(n_rows, n_columns)) return rc;
    if (params->c != 0.0 && !n_frames) return capi_fail(DSP_EINVAL, "params->c != 0 without n_frames");
    if (n_rows == 0) return DSP_OK;
    if (!d_scores) return capi_fail(DSP_EINVAL, "d_scores is NULL");
    if (!d_out) return capi_fail(DSP_EINVAL, "d_out is NULL");
    if (n_frames)
        if (const int rc = check_frames(n_frames, n_rows)) return rc;
    if (const int rc = dsp::check_trial_count(n_rows, n_columns)) return rc;
    if (const int rc = dsp::check_device(c->device)) return rc;
    DSP_ON_DEVICE(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (!n_frames) {
        DSP_CAPI_HIP(dsp::launch_calibration_apply(d_scores, nullptr, n_rows, n_columns, *params, d_out, st));
        return DSP_OK;
    }
    const size_t bytes = (size_t)n_rows * sizeof(double);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(c->spans, bytes, slot)) return rc;
    double *h_duration = static_cast<double *>(slot.h());
    for (long r = 0; r < n_rows; ++r) h_duration[r] = duration_term(n_frames[r]);
    DSP_CAPI_HIP(slot.upload(bytes, st));
    DSP_CAPI_HIP(dsp::launch_calibration_apply(d_scores, static_cast<const double *>(slot.d()), n_rows, n_columns, *params, d_out, st));
    return DSP_OK;
}

}  // extern "C"
