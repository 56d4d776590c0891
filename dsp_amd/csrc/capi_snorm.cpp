// capi_snorm.cpp -- the C ABI of cohort normalisation (include/dsp_amd.h dsp_cohort_stats_device, dsp_score_normalize_device;
// DESIGN.md 3.24): argument checks, all of them before a device is touched and in the order the header states, then the launches of
// snorm_kernels.hip.  The kernels keep everything they need in LDS: no workspace, no state between calls, and so no handle.
#include <cmath>

#include "capi_util.hpp"
#include "snorm_kernels.hpp"

using dsp::capi_fail;

static_assert(sizeof(dsp_cohort_stat) == 32, "dsp_cohort_stat is 32 bytes (dsp_amd/lib.py CohortStat)");
static_assert(sizeof(dsp_snorm_config) == 16, "dsp_snorm_config is 16 bytes (dsp_amd/lib.py SnormConfig)");

extern "C" {

int dsp_cohort_stats_device(int device, const float *d_cohort, long n_rows, long n_cols, int axis, int top_k, dsp_cohort_stat *d_stats,
                            void *stream)
{
    if (device < 0) return capi_fail(DSP_EINVAL, "device index out of range");
    if (axis != DSP_COHORT_PER_ROW && axis != DSP_COHORT_PER_COLUMN) return capi_fail(DSP_EINVAL, "axis must be DSP_COHORT_PER_ROW or DSP_COHORT_PER_COLUMN");
    if (top_k < 0 || top_k > dsp::kSnormMaxTopK) return capi_fail(DSP_EINVAL, "top_k must be 0 .. 2^22, got " + std::to_string(top_k));
    if (n_rows < 0 || n_cols < 0) return capi_fail(DSP_EINVAL, "n_rows or n_cols < 0");
    const long vectors = axis == DSP_COHORT_PER_ROW ? n_rows : n_cols, length = axis == DSP_COHORT_PER_ROW ? n_cols : n_rows;
    if (vectors > dsp::kSnormMaxVectors) return capi_fail(DSP_EINVAL, "more than 2^30 vectors in one call");
    if (vectors == 0) return DSP_OK;
    if (length < 1 || length > dsp::kSnormMaxLength) return capi_fail(DSP_EINVAL, "the cohort length must be 1 .. 2^22, got " + std::to_string(length));
    if (!d_cohort) return capi_fail(DSP_EINVAL, "d_cohort is NULL");
    if (!d_stats) return capi_fail(DSP_EINVAL, "d_stats is NULL");
    if (const int rc = dsp::check_device(device)) return rc;
    DSP_ON_DEVICE(device);
    DSP_CAPI_HIP(dsp::launch_cohort_stats(d_cohort, n_rows, n_cols, axis, top_k, d_stats, (hipStream_t)stream));
    return DSP_OK;
}

int dsp_score_normalize_device(int device, const float *d_scores, long n_rows, long n_cols, const dsp_cohort_stat *d_row_stats,
                               const dsp_cohort_stat *d_col_stats, const dsp_snorm_config *cfg, float *d_out, void *stream)
{
    if (device < 0) return capi_fail(DSP_EINVAL, "device index out of range");
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_snorm_config is NULL");
    if (cfg->mode != DSP_NORM_Z && cfg->mode != DSP_NORM_T && cfg->mode != DSP_NORM_S)
        return capi_fail(DSP_EINVAL, "dsp_snorm_config: mode must be DSP_NORM_Z, DSP_NORM_T or DSP_NORM_S");
    if (!(std::isfinite(cfg->std_floor) && cfg->std_floor >= 0.0)) return capi_fail(DSP_EINVAL, "dsp_snorm_config: std_floor must be finite and >= 0");
    if (n_rows < 0 || n_cols < 0) return capi_fail(DSP_EINVAL, "n_rows or n_cols < 0");
    if (n_rows > dsp::kSnormMaxVectors || n_cols > dsp::kSnormMaxVectors) return capi_fail(DSP_EINVAL, "more than 2^30 rows or columns");
    if (n_rows == 0 || n_cols == 0) return DSP_OK;
    if (!d_scores) return capi_fail(DSP_EINVAL, "d_scores is NULL");
    if (!d_out) return capi_fail(DSP_EINVAL, "d_out is NULL");
    if (cfg->mode != DSP_NORM_Z && !d_row_stats) return capi_fail(DSP_EINVAL, "d_row_stats is NULL: DSP_NORM_T and DSP_NORM_S need it");
    if (cfg->mode != DSP_NORM_T && !d_col_stats) return capi_fail(DSP_EINVAL, "d_col_stats is NULL: DSP_NORM_Z and DSP_NORM_S need it");
    if (const int rc = dsp::check_device(device)) return rc;
    DSP_ON_DEVICE(device);
    DSP_CAPI_HIP(dsp::launch_score_normalize(d_scores, n_rows, n_cols, d_row_stats, d_col_stats, cfg->mode, cfg->std_floor, d_out, (hipStream_t)stream));
    return DSP_OK;
}

}  // extern "C"
