// capi_trials.cpp -- the C ABI of labelled trials (include/dsp_amd.h dsp_trial*): argument checks, all of them before a
// device is touched, the host-only target lists and pair count, the evaluator's grow-only workspace and the labels that travel
// through its ring to the kernels of trial_kernels.hip.
#include "capi_util.hpp"
#include "trial_kernels.hpp"

using dsp::capi_fail;

static_assert(sizeof(dsp_trial_column) == 80, "dsp_trial_column is 80 bytes (dsp_amd/lib.py TRIAL_COLUMN_DTYPE)");

struct dsp_trial_evaluator : dsp::StageHandle {};      // ws: TrialWorkspace (trial_kernels.hpp); spans: target_offsets | truth | target_rows

namespace {

// P_s of every column: counts[s + 1] (counts[0] stays 0) -> the number of targets
long count_targets(const int *truth, long n_rows, std::vector<long> &counts)
{
    long total = 0;
    for (long r = 0; r < n_rows; ++r)
        if (truth[r] >= 0) { ++counts[(size_t)truth[r] + 1]; ++total; }
    return total;
}

}  // namespace

extern "C" {

long dsp_trials_target_offsets(const int *truth, long n_rows, long n_columns, long *target_offsets, long *target_rows)
{
    if (const int rc = dsp::check_score_shape(n_rows, n_columns)) return rc;
    if (n_rows > 0 && !truth) return capi_fail(DSP_EINVAL, "truth is NULL");
    if (const int rc = dsp::check_truth(truth, n_rows, n_columns)) return rc;
    std::vector<long> at((size_t)n_columns + 1, 0);
    const long total = count_targets(truth, n_rows, at);
    for (long s = 0; s < n_columns; ++s) at[(size_t)s + 1] += at[(size_t)s];
    if (target_offsets) std::copy(at.begin(), at.end(), target_offsets);
    if (target_rows)
        for (long r = 0; r < n_rows; ++r)
            if (truth[r] >= 0) target_rows[at[(size_t)truth[r]]++] = r;
    return total;
}

long dsp_trials_pairs(const int *truth, long n_rows, long n_columns)
{
    if (const int rc = dsp::check_score_shape(n_rows, n_columns)) return rc;
    if (n_rows > 0 && !truth) return capi_fail(DSP_EINVAL, "truth is NULL");
    if (const int rc = dsp::check_truth(truth, n_rows, n_columns)) return rc;
    std::vector<long> counts((size_t)n_columns + 1, 0);
    count_targets(truth, n_rows, counts);
    long pairs = 0;                      // (the P_s add up to n_rows < 2^31 at most: below 2^62)
    for (long s = 0; s < n_columns; ++s) pairs += counts[(size_t)s + 1] * (n_rows - counts[(size_t)s + 1]);
    return pairs;
}

int dsp_trial_evaluator_create(int device, dsp_trial_evaluator **out) { return dsp::create_on_host(device, out); }

void dsp_trial_evaluator_destroy(dsp_trial_evaluator *e) { dsp::destroy(e); }

int dsp_trials_evaluate_device(dsp_trial_evaluator *e, const float *d_scores, long n_rows, long n_columns, const int *truth, const dsp_trials_config *cfg,
                               dsp_trial_column *d_columns, long *d_sweep_tp, long *d_sweep_fp, int *d_fa_above, int *d_fa_equal, void *stream)
{
    if (!e) return capi_fail(DSP_EINVAL, "evaluator is NULL");
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_trials_config is NULL");
    if (cfg->n_thresholds < dsp::kTrialMinThresholds || cfg->n_thresholds > dsp::kTrialMaxThresholds)
        return capi_fail(DSP_EINVAL, "dsp_trials_config: n_thresholds must be 2 .. 1024, got " + std::to_string(cfg->n_thresholds));
    if (const int rc = dsp::check_score_shape(n_rows, n_columns)) return rc;
    if (!d_columns && !d_sweep_tp && !d_sweep_fp && !d_fa_above && !d_fa_equal) return capi_fail(DSP_EINVAL, "every output is NULL");
    if (n_rows == 0) return DSP_OK;
    if (!d_scores) return capi_fail(DSP_EINVAL, "d_scores is NULL");
    if (!truth) return capi_fail(DSP_EINVAL, "truth is NULL");
    if (const int rc = dsp::check_truth(truth, n_rows, n_columns)) return rc;
    if (const int rc = dsp::check_trial_count(n_rows, n_columns)) return rc;
    std::vector<long> at((size_t)n_columns + 1, 0);
    const long targets = count_targets(truth, n_rows, at);
    const bool want_pairs = d_columns || d_fa_above || d_fa_equal;
    if (want_pairs) {
        long pairs = 0;
        for (long s = 0; s < n_columns; ++s) pairs += at[(size_t)s + 1] * (n_rows - at[(size_t)s + 1]);
        if (pairs > dsp::kTrialMaxPairs)
            return capi_fail(DSP_EINVAL, std::to_string(pairs) + " pairs of a target and a non-target: d_columns and the ROC counts take 2^46 at most");
    }
    for (long s = 0; s < n_columns; ++s) at[(size_t)s + 1] += at[(size_t)s];
    if (const int rc = dsp::check_device(e->device)) return rc;
    DSP_ON_DEVICE(e->device);
    hipStream_t st = (hipStream_t)stream;
    // target_offsets, S + 1 longs | truth, T ints | target_rows, one int per target
    const size_t n1 = (size_t)n_columns + 1, bytes = n1 * sizeof(long) + ((size_t)n_rows + (size_t)targets) * sizeof(int);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(e->spans, bytes, slot)) return rc;
    long *h_offsets = static_cast<long *>(slot.h());
    int *h_truth = reinterpret_cast<int *>(h_offsets + n1), *h_rows = h_truth + n_rows;
    std::copy(at.begin(), at.end(), h_offsets);
    std::memcpy(h_truth, truth, (size_t)n_rows * sizeof(int));
    for (long r = 0; r < n_rows; ++r)
        if (truth[r] >= 0) h_rows[at[(size_t)truth[r]]++] = (int)r;
    if (e->ws.reserve(dsp::trial_workspace_bytes(n_columns, cfg->n_thresholds, targets)) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc of the evaluator's workspace");
    const dsp::TrialWorkspace ws = dsp::trial_carve(e->ws.get(), n_columns, cfg->n_thresholds, targets);
    DSP_CAPI_HIP(slot.upload(bytes, st));
    const long *d_offsets = static_cast<const long *>(slot.d());
    const int *d_truth = reinterpret_cast<const int *>(d_offsets + n1);
    dsp::TrialCall call{d_scores, d_truth, d_offsets, d_truth + n_rows, n_rows, n_columns, targets, cfg->n_thresholds, d_columns, d_sweep_tp, d_sweep_fp,
                        d_fa_above, d_fa_equal};
    DSP_CAPI_HIP(dsp::launch_trials(call, ws, st));
    return DSP_OK;
}

}  // extern "C"
