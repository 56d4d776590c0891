// capi_ubm.cpp -- the C ABI of UBM training and of the GMM quantiser (include/dsp_amd.h dsp_ubm_*, dsp_gmm_quantize):
// argument checks, the trainer's grow-only workspace, the initial model, the enqueueing of the EM iterations of ubm_kernels.hip and the
// one synchronisation that reads the result back.  The E-step model is a GmmModel (gmm_model.hpp), as capi_enroll.cpp's UBM is.
// Behind it the k-means start on the same trainer (dsp_kmeans_*): seeding, Lloyd and the restarts, kmeans_kernels.hip.
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>

#include "capi_util.hpp"
#include "kmeans_kernels.hpp"
#include "ubm_kernels.hpp"

using dsp::capi_fail;

struct dsp_ubm_trainer : dsp::Handle {
    int k = 0, d = 0;
    dsp::DeviceBuf<double> partials;     // grow-only: the groups' partials, the supers' behind them
    dsp::DeviceBuf<double> state;        // grow-only: the float64 parameters, lower_bounds[max_iter] behind them
    dsp::DeviceBuf<float> model;         // the float32 E-step model
    dsp::DeviceBuf<dsp::UbmCtrl> ctrl;
    // k-means (grow-only as well)
    dsp::DeviceBuf<double> km_centres;   // the float64 centres [k][d], the final counts [k] behind them
    dsp::DeviceBuf<int> km_labels;       // [n], where the caller asks for none
    dsp::DeviceBuf<dsp::KmeansCtrl> km_ctrl;
    dsp::DeviceBuf<float> km_m;          // seeding: [n] nearest squared distances
    dsp::DeviceBuf<double> km_sums;      // seeding: the draws, then per trial the chunks', groups' and supers' sums
    dsp::DeviceBuf<dsp::KmeansSeedCtrl> km_seed_ctrl;
};

namespace {

// iterations enqueued between two looks at the stop flag: a fit that stops early wastes at most this many empty iterations
constexpr int kIterationsPerLook = 32;
constexpr long kMaxRows = 1L << 40;

struct HostModel {
    std::vector<double> params;          // w[k], mu[k][d], var[k][d], log_const[k]
    std::vector<float> model;            // log_const[k], c[k][d], ic[k][d]
};

HostModel host_model(int k, int d, const double *w, const double *mu, const double *var)
{
    HostModel m;
    m.params.resize(dsp::ubm_param_doubles(k, d));
    const dsp::UbmParams<double> p{m.params.data(), k, d};
    const size_t kd = (size_t)k * d;
    std::vector<double> inv_var(kd);
    for (int i = 0; i < k; ++i) {
        double log_det = 0.0;
        for (int j = 0; j < d; ++j) log_det += std::log(2.0 * M_PI * var[(size_t)i * d + j]);
        p.w()[i] = w[i];
        p.log_const()[i] = std::log(w[i]) - 0.5 * log_det;
    }
    for (size_t i = 0; i < kd; ++i) {
        p.mu()[i] = mu[i];
        p.var()[i] = var[i];
        inv_var[i] = 1.0 / var[i];
    }
    m.model = dsp::pack_gmm_model(k, d, p.log_const(), mu, inv_var.data());
    return m;
}

// kIterationsPerLook iterations at a time through launch(first, count) (a DSP_* code: the caller words its failure), after each batch
// the device control word into *end and one synchronisation, until end->done or max_iter
template <class Ctrl, class Launch>
int run_until_done(int max_iter, const Ctrl *d_ctrl, Ctrl *end, hipStream_t stream, Launch &&launch)
{
    for (int first = 0; first < max_iter && !end->done; first += kIterationsPerLook) {
        const int count = max_iter - first < kIterationsPerLook ? max_iter - first : kIterationsPerLook;
        if (const int rc = launch(first, count)) return rc;
        DSP_CAPI_HIP(hipMemcpyAsync(end, d_ctrl, sizeof(*end), hipMemcpyDeviceToHost, stream));
        DSP_CAPI_HIP(hipStreamSynchronize(stream));
    }
    return DSP_OK;
}

int reserve_em(dsp_ubm_trainer *t, int k, long n, int max_iter, size_t stride)
{
    const size_t n_params = dsp::ubm_param_doubles(k, t->d);
    if (t->partials.reserve((size_t)(dsp::ubm_groups(n) + dsp::ubm_supers(n)) * stride * sizeof(double)) != hipSuccess ||
        t->state.reserve((n_params + (size_t)max_iter) * sizeof(double)) != hipSuccess ||
        t->model.reserve(dsp::gmm_model_floats(t->k, t->d) * sizeof(float)) != hipSuccess || t->ctrl.reserve(sizeof(dsp::UbmCtrl)) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc of the trainer's workspace");
    return DSP_OK;
}

// EM from the parameters and the float32 model that the trainer's workspace holds (reserve_em went before): up to max_iter iterations,
// the parameters after the last one into `params` (ubm_param_doubles), lower_bounds[0 .. n_iter) into `lower_bounds`
int run_em_from_device(dsp_ubm_trainer *t, int k, const float *d_feats, long n, int max_iter, double tol, double reg_covar, double *params, double *lower_bounds,
                       int *n_iter, int *converged, hipStream_t stream)
{
    const int d = t->d;
    const size_t stride = dsp::ubm_partial_doubles(k, d), n_params = dsp::ubm_param_doubles(k, d);
    const long n_groups = dsp::ubm_groups(n);
    const dsp::UbmCtrl start{0, 0, 0, 0, -std::numeric_limits<double>::infinity()};
    DSP_CAPI_HIP(hipMemcpyAsync(t->ctrl, &start, sizeof(start), hipMemcpyHostToDevice, stream));
    dsp::UbmFit fit{d_feats, n, t->state, dsp::GmmModelOut{t->model, k, d}, t->partials, t->partials.get() + (size_t)n_groups * stride, t->state.get() + n_params,
                    t->ctrl, tol, reg_covar};
    dsp::UbmCtrl end = start;
    if (const int rc = run_until_done(max_iter, t->ctrl.get(), &end, stream, [&](int first, int count) -> int {
            DSP_CAPI_HIP(dsp::launch_ubm_iterations(fit, first, count, stream));
            return DSP_OK;
        }))
        return rc;
    DSP_CAPI_HIP(hipMemcpyAsync(params, t->state, n_params * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (lower_bounds) DSP_CAPI_HIP(hipMemcpyAsync(lower_bounds, fit.lower_bounds, (size_t)end.n_iter * sizeof(double), hipMemcpyDeviceToHost, stream));
    DSP_CAPI_HIP(hipStreamSynchronize(stream));
    *n_iter = end.n_iter;
    *converged = end.converged;
    return DSP_OK;
}

// EM from (w, mu, var) on the trainer's device (current).  k may be below the trainer's (the k = 1 pass of the row start).
int run_em(dsp_ubm_trainer *t, int k, const float *d_feats, long n, const double *w, const double *mu, const double *var, int max_iter, double tol,
           double reg_covar, double *params, double *lower_bounds, int *n_iter, int *converged, hipStream_t stream)
{
    const int d = t->d;
    if (const int rc = reserve_em(t, k, n, max_iter, dsp::ubm_partial_doubles(k, d))) return rc;
    const HostModel m = host_model(k, d, w, mu, var);
    DSP_CAPI_HIP(hipMemcpyAsync(t->state, m.params.data(), dsp::ubm_param_doubles(k, d) * sizeof(double), hipMemcpyHostToDevice, stream));
    DSP_CAPI_HIP(hipMemcpyAsync(t->model, m.model.data(), m.model.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    return run_em_from_device(t, k, d_feats, n, max_iter, tol, reg_covar, params, lower_bounds, n_iter, converged, stream);
}

int check_rows(const dsp_ubm_trainer *t, const float *d_feats, long n)
{
    if (!t) return capi_fail(DSP_EINVAL, "trainer is NULL");
    if (!d_feats) return capi_fail(DSP_EINVAL, "d_feats is NULL");
    if (n < t->k) return capi_fail(DSP_EINVAL, "n must be at least k = " + std::to_string(t->k) + " rows, got " + std::to_string(n));
    if (n > kMaxRows) return capi_fail(DSP_EINVAL, "n: at most 2^40 rows per call");
    return DSP_OK;
}

int check_reg_covar(double reg_covar)
{
    if (!(reg_covar >= 0.0) || !std::isfinite(reg_covar)) return capi_fail(DSP_EINVAL, "reg_covar must be >= 0 and finite");
    return DSP_OK;
}

// the rows' global variance per dimension + reg_covar: one k = 1 iteration from the k = 1 start (the middle row, variance 1)
int global_variance(dsp_ubm_trainer *t, const float *d_feats, long n, double reg_covar, std::vector<double> &variance, hipStream_t stream)
{
    const int d = t->d;
    // centred on the middle row (the k = 1 start's own mean), not on 0: rows far from the origin would lose their variance to float32
    std::vector<float> middle((size_t)d);
    DSP_CAPI_HIP(hipMemcpyAsync(middle.data(), d_feats + (size_t)(n / 2) * d, (size_t)d * sizeof(float), hipMemcpyDeviceToHost, stream));
    DSP_CAPI_HIP(hipStreamSynchronize(stream));
    std::vector<double> one_mu(middle.begin(), middle.end()), one_var((size_t)d, 1.0), params(dsp::ubm_param_doubles(1, d));
    const double one_w = 1.0;
    int n_iter = 0, converged = 0;
    if (const int rc = run_em(t, 1, d_feats, n, &one_w, one_mu.data(), one_var.data(), 1, 0.0, reg_covar, params.data(), nullptr, &n_iter, &converged, stream))
        return rc;
    const dsp::UbmParams<const double> p{params.data(), 1, d};
    variance.assign(p.var(), p.var() + d);
    return DSP_OK;
}

// the library's start: means = rows floor((i + 0.5) n / k), variances = the rows' global variance + reg_covar, weights 1 / k
int init_rows(dsp_ubm_trainer *t, const float *d_feats, long n, double reg_covar, double *weights, double *means, double *variances, hipStream_t stream)
{
    const int k = t->k, d = t->d;
    std::vector<double> variance;
    if (const int rc = global_variance(t, d_feats, n, reg_covar, variance, stream)) return rc;
    std::vector<float> rows((size_t)k * d);
    for (int i = 0; i < k; ++i) {
        const long row = (long)(((__int128)(2 * i + 1) * n) / (2 * k));
        DSP_CAPI_HIP(hipMemcpyAsync(rows.data() + (size_t)i * d, d_feats + (size_t)row * d, (size_t)d * sizeof(float), hipMemcpyDeviceToHost, stream));
    }
    DSP_CAPI_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < k; ++i) {
        weights[i] = 1.0 / k;
        for (int j = 0; j < d; ++j) {
            means[(size_t)i * d + j] = (double)rows[(size_t)i * d + j];
            variances[(size_t)i * d + j] = variance[(size_t)j];
        }
    }
    return DSP_OK;
}

// --- the k-means start (include/dsp_amd.h dsp_kmeans_*) ---

int check_kmeans_numbers(int max_iter, double tol, double reg_covar, const char *who)
{
    if (max_iter < 1) return capi_fail(DSP_EINVAL, std::string(who) + "max_iter must be >= 1, got " + std::to_string(max_iter));
    if (!(tol >= 0.0) || !std::isfinite(tol)) return capi_fail(DSP_EINVAL, std::string(who) + "tol must be >= 0 and finite");
    return check_reg_covar(reg_covar);
}

// greedy k-means++ on the trainer's device (current) -> rows[k]
int seed_rows(dsp_ubm_trainer *t, const float *d_feats, long n, uint64_t seed, long *rows, hipStream_t stream)
{
    const int k = t->k, d = t->d, trials = dsp::kmeans_trials(k);
    const long n_chunks = dsp::kmeans_chunks(n), n_groups = dsp::ubm_groups(n), n_supers = dsp::ubm_supers(n);
    const size_t n_u = (size_t)k * dsp::kKmeansMaxTrials;
    if (t->km_m.reserve((size_t)n * sizeof(float)) != hipSuccess ||
        t->km_sums.reserve((n_u + (size_t)trials * (size_t)(n_chunks + n_groups + n_supers)) * sizeof(double)) != hipSuccess ||
        t->km_seed_ctrl.reserve(sizeof(dsp::KmeansSeedCtrl)) != hipSuccess)
        return capi_fail(DSP_ENOMEM, "hipMalloc of the trainer's seeding workspace");
    std::vector<double> u(n_u, 0.0);
    for (int j = 0; j < k; ++j)
        for (int tr = 0; tr < trials; ++tr) u[(size_t)j * dsp::kKmeansMaxTrials + tr] = dsp::kmeans_draw(seed, j, tr);
    long row0 = (long)(u[0] * (double)n);
    if (row0 >= n) row0 = n - 1;
    dsp::KmeansSeedCtrl ctrl{};
    ctrl.cand[0] = row0;
    DSP_CAPI_HIP(hipMemcpyAsync(t->km_sums, u.data(), n_u * sizeof(double), hipMemcpyHostToDevice, stream));
    DSP_CAPI_HIP(hipMemcpyAsync(t->km_seed_ctrl, &ctrl, sizeof(ctrl), hipMemcpyHostToDevice, stream));
    double *chunks = t->km_sums.get() + n_u, *groups = chunks + (size_t)trials * n_chunks, *supers = groups + (size_t)trials * n_groups;
    DSP_CAPI_HIP(dsp::launch_kmeans_seeding(dsp::KmeansSeed{d_feats, n, k, d, trials, t->km_m, chunks, groups, supers, t->km_sums, t->km_seed_ctrl}, row0, stream));
    dsp::KmeansSeedCtrl end{};
    DSP_CAPI_HIP(hipMemcpyAsync(&end, t->km_seed_ctrl, sizeof(end), hipMemcpyDeviceToHost, stream));
    DSP_CAPI_HIP(hipStreamSynchronize(stream));
    if (end.failed == 1)
        return capi_fail(DSP_EINVAL, "d_feats holds fewer than k = " + std::to_string(k) + " distinct rows: " + std::to_string(end.failed_step) +
                                         " centres chosen, every row sits on one of them");
    if (end.failed) return capi_fail(DSP_EHIP, "k-means++ seeding: no row under a positive sum at step " + std::to_string(end.failed_step));
    for (int i = 0; i < k; ++i) rows[i] = end.rows[i];
    return DSP_OK;
}

int reserve_kmeans(dsp_ubm_trainer *t, long n, int em_max_iter, bool own_labels)
{
    const int k = t->k, d = t->d;
    if (const int rc = reserve_em(t, k, n, em_max_iter, dsp::kmeans_partial_doubles(k, d))) return rc;
    if (t->km_centres.reserve(((size_t)k * d + k) * sizeof(double)) != hipSuccess || t->km_ctrl.reserve(sizeof(dsp::KmeansCtrl)) != hipSuccess ||
        (own_labels && t->km_labels.reserve((size_t)n * sizeof(int)) != hipSuccess))
        return capi_fail(DSP_ENOMEM, "hipMalloc of the trainer's k-means workspace");
    return DSP_OK;
}

// Lloyd from centres0 (reserve_kmeans went before) and the final pass: the GMM start is left in the trainer's device parameters and
// float32 model, the centres and counts in km_centres; `end` says how it stopped
int run_lloyd(dsp_ubm_trainer *t, const float *d_feats, long n, const double *centres0, int max_iter, double shift_limit, double reg_covar, int *d_labels,
              dsp::KmeansCtrl *end, hipStream_t stream)
{
    const int k = t->k, d = t->d;
    const size_t kd = (size_t)k * d, stride = dsp::kmeans_partial_doubles(k, d);
    const long n_groups = dsp::ubm_groups(n);
    std::vector<float> c(centres0, centres0 + kd);                   // each rounded once
    const dsp::GmmModelOut model{t->model, k, d};
    int *labels = d_labels ? d_labels : t->km_labels.get();
    const dsp::KmeansCtrl start{};
    DSP_CAPI_HIP(hipMemcpyAsync(t->km_centres, centres0, kd * sizeof(double), hipMemcpyHostToDevice, stream));
    DSP_CAPI_HIP(hipMemcpyAsync(model.means(), c.data(), kd * sizeof(float), hipMemcpyHostToDevice, stream));
    DSP_CAPI_HIP(hipMemcpyAsync(t->km_ctrl, &start, sizeof(start), hipMemcpyHostToDevice, stream));
    DSP_CAPI_HIP(hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(int), stream));      // -1: every row changes in the first iteration
    const dsp::KmeansFit fit{d_feats, n, t->km_centres, model, labels, t->partials, t->partials.get() + (size_t)n_groups * stride, t->km_ctrl, shift_limit, max_iter,
                             reg_covar, t->state, t->km_centres.get() + kd};
    *end = start;
    if (const int rc = run_until_done(max_iter, t->km_ctrl.get(), end, stream, [&](int first, int count) -> int {
            DSP_CAPI_HIP(dsp::launch_kmeans_iterations(fit, first, count, stream));
            return DSP_OK;
        }))
        return rc;
    DSP_CAPI_HIP(dsp::launch_kmeans_final(fit, stream));
    DSP_CAPI_HIP(hipMemcpyAsync(end, t->km_ctrl, sizeof(*end), hipMemcpyDeviceToHost, stream));
    DSP_CAPI_HIP(hipStreamSynchronize(stream));                       // (also: `c` and `start` are read by then)
    return DSP_OK;
}

// tol * mean_d var_d(x): sklearn's _tolerance
int shift_limit_of(dsp_ubm_trainer *t, const float *d_feats, long n, double tol, double *limit, hipStream_t stream)
{
    std::vector<double> variance;
    if (const int rc = global_variance(t, d_feats, n, 0.0, variance, stream)) return rc;
    double sum = 0.0;
    for (double v : variance) sum += v;
    *limit = tol * (sum / (double)variance.size());
    return DSP_OK;
}

int check_ubm_result(const dsp_ubm_result *result)
{
    if (!result || !result->weights || !result->variances || !result->lower_bounds) return capi_fail(DSP_EINVAL, "dsp_ubm_result and its arrays must not be NULL");
    return dsp::check_gmm_float_arrays(&result->gmm, "dsp_ubm_result");      // (k and d are the call's to write)
}

void write_ubm_result(dsp_ubm_result *result, int k, int d, const std::vector<double> &params, int n_iter, int converged)
{
    const size_t kd = (size_t)k * d;
    const dsp::UbmParams<const double> p{params.data(), k, d};
    // the caller's arrays behind the const pointers of dsp_gmm_float_params are the result's to write
    double *log_consts = const_cast<double *>(result->gmm.log_consts), *means = const_cast<double *>(result->gmm.means);
    double *inv_covs = const_cast<double *>(result->gmm.inv_covs);
    for (int i = 0; i < k; ++i) {
        result->weights[i] = p.w()[i];
        log_consts[i] = p.log_const()[i];
    }
    for (size_t i = 0; i < kd; ++i) {
        means[i] = p.mu()[i];
        result->variances[i] = p.var()[i];
        inv_covs[i] = 1.0 / p.var()[i];
    }
    result->gmm.k = k;
    result->gmm.d = d;
    result->n_iter = n_iter;
    result->converged = converged;
}

}  // namespace

extern "C" {

int dsp_ubm_trainer_create(int device, int k, int d, dsp_ubm_trainer **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (k < 1 || k > dsp::kGmmMaxK) return capi_fail(DSP_EINVAL, "k must be 1 .. 64, got " + std::to_string(k));
    if (d < 1 || d > dsp::kGmmMaxD) return capi_fail(DSP_EINVAL, "d must be 1 .. 16, got " + std::to_string(d));
    // nothing is allocated here and no device is touched: the workspace grows in the first call that trains, which is also where a
    // device that does not exist is reported
    return dsp::create_on_host(device, out, [&](dsp_ubm_trainer &t) {
        t.k = k;
        t.d = d;
        return DSP_OK;
    });
}

void dsp_ubm_trainer_destroy(dsp_ubm_trainer *t) { dsp::destroy(t); }

int dsp_ubm_init_rows_device(dsp_ubm_trainer *t, const float *d_feats, long n, double reg_covar, double *weights, double *means, double *variances,
                             void *stream)
{
    if (const int rc = check_rows(t, d_feats, n)) return rc;
    if (const int rc = check_reg_covar(reg_covar)) return rc;
    if (!weights || !means || !variances) return capi_fail(DSP_EINVAL, "weights, means and variances must not be NULL");
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    return init_rows(t, d_feats, n, reg_covar, weights, means, variances, (hipStream_t)stream);
}

int dsp_ubm_train_device(dsp_ubm_trainer *t, const float *d_feats, long n, const dsp_ubm_init *init, const dsp_ubm_config *cfg, dsp_ubm_result *result,
                         void *stream)
{
    if (const int rc = check_rows(t, d_feats, n)) return rc;
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_ubm_config is NULL");
    if (cfg->max_iter < 1) return capi_fail(DSP_EINVAL, "dsp_ubm_config: max_iter must be >= 1, got " + std::to_string(cfg->max_iter));
    if (!(cfg->tol >= 0.0)) return capi_fail(DSP_EINVAL, "dsp_ubm_config: tol must be >= 0");
    if (const int rc = check_reg_covar(cfg->reg_covar)) return rc;
    const int k = t->k, d = t->d;
    const size_t kd = (size_t)k * d;
    if (init) {
        if (!init->weights || !init->means || !init->variances) return capi_fail(DSP_EINVAL, "dsp_ubm_init: weights, means and variances must not be NULL");
        double sum = 0.0;
        for (int i = 0; i < k; ++i) {
            if (!std::isfinite(init->weights[i])) return capi_fail(DSP_EINVAL, "dsp_ubm_init: weights must be finite");
            if (!(init->weights[i] > 0.0)) return capi_fail(DSP_EINVAL, "dsp_ubm_init: weights must be > 0 (component " + std::to_string(i) + ")");
            sum += init->weights[i];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-6)) return capi_fail(DSP_EINVAL, "dsp_ubm_init: weights must sum to 1 within 1e-6");
        for (size_t i = 0; i < kd; ++i) {
            if (!std::isfinite(init->means[i]) || !std::isfinite(init->variances[i])) return capi_fail(DSP_EINVAL, "dsp_ubm_init: means and variances must be finite");
            if (!(init->variances[i] > 0.0)) return capi_fail(DSP_EINVAL, "dsp_ubm_init: variances must be > 0 (component " + std::to_string(i / d) + ")");
        }
    }
    if (const int rc = check_ubm_result(result)) return rc;
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    std::vector<double> start;
    const double *w, *mu, *var;
    if (init) {
        w = init->weights; mu = init->means; var = init->variances;
    } else {
        start.resize(dsp::ubm_param_doubles(k, d));
        const dsp::UbmParams<double> p{start.data(), k, d};
        if (const int rc = init_rows(t, d_feats, n, cfg->reg_covar, p.w(), p.mu(), p.var(), (hipStream_t)stream)) return rc;
        w = p.w(); mu = p.mu(); var = p.var();
    }
    std::vector<double> params(dsp::ubm_param_doubles(k, d));
    int n_iter = 0, converged = 0;
    if (const int rc = run_em(t, k, d_feats, n, w, mu, var, cfg->max_iter, cfg->tol, cfg->reg_covar, params.data(), result->lower_bounds, &n_iter, &converged,
                              (hipStream_t)stream))
        return rc;
    write_ubm_result(result, k, d, params, n_iter, converged);
    return DSP_OK;
}

int dsp_kmeans_seed_device(dsp_ubm_trainer *t, const float *d_feats, long n, uint64_t seed, long *rows, void *stream)
{
    if (const int rc = check_rows(t, d_feats, n)) return rc;
    if (!rows) return capi_fail(DSP_EINVAL, "rows is NULL");
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    return seed_rows(t, d_feats, n, seed, rows, (hipStream_t)stream);
}

int dsp_kmeans_fit_device(dsp_ubm_trainer *t, const float *d_feats, long n, const double *centres0, const dsp_kmeans_config *cfg, dsp_kmeans_result *result,
                          void *stream)
{
    if (const int rc = check_rows(t, d_feats, n)) return rc;
    if (!centres0) return capi_fail(DSP_EINVAL, "centres0 is NULL");
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_kmeans_config is NULL");
    if (const int rc = check_kmeans_numbers(cfg->max_iter, cfg->tol, cfg->reg_covar, "dsp_kmeans_config: ")) return rc;
    const int k = t->k, d = t->d;
    const size_t kd = (size_t)k * d;
    for (size_t i = 0; i < kd; ++i)
        if (!std::isfinite(centres0[i]) || std::fabs(centres0[i]) > (double)std::numeric_limits<float>::max())
            return capi_fail(DSP_EINVAL, "centres0 must be finite (centre " + std::to_string(i / d) + ")");
    if (!result || !result->centres || !result->counts || !result->weights || !result->means || !result->variances)
        return capi_fail(DSP_EINVAL, "dsp_kmeans_result and its centres, counts, weights, means and variances must not be NULL");
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t s = (hipStream_t)stream;
    double limit = 0.0;
    if (const int rc = shift_limit_of(t, d_feats, n, cfg->tol, &limit, s)) return rc;
    if (const int rc = reserve_kmeans(t, n, 1, !result->d_labels)) return rc;
    dsp::KmeansCtrl end{};
    if (const int rc = run_lloyd(t, d_feats, n, centres0, cfg->max_iter, limit, cfg->reg_covar, result->d_labels, &end, s)) return rc;
    std::vector<double> params(dsp::ubm_param_doubles(k, d)), counts((size_t)k);
    DSP_CAPI_HIP(hipMemcpyAsync(result->centres, t->km_centres, kd * sizeof(double), hipMemcpyDeviceToHost, s));
    DSP_CAPI_HIP(hipMemcpyAsync(counts.data(), t->km_centres.get() + kd, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, s));
    DSP_CAPI_HIP(hipMemcpyAsync(params.data(), t->state, params.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    DSP_CAPI_HIP(hipStreamSynchronize(s));
    const dsp::UbmParams<const double> p{params.data(), k, d};
    for (int i = 0; i < k; ++i) {
        result->counts[i] = (long)counts[i];
        result->weights[i] = p.w()[i];
    }
    for (size_t i = 0; i < kd; ++i) {
        result->means[i] = p.mu()[i];
        result->variances[i] = p.var()[i];
    }
    result->inertia = end.inertia;
    result->n_iter = end.n_iter;
    result->stop = end.reason;
    result->n_empty = end.n_empty;
    return DSP_OK;
}

int dsp_kmeans_train_ubm_device(dsp_ubm_trainer *t, const float *d_feats, long n, const dsp_kmeans_ubm_config *cfg, dsp_ubm_result *result,
                                dsp_kmeans_ubm_report *report, void *stream)
{
    if (const int rc = check_rows(t, d_feats, n)) return rc;
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_kmeans_ubm_config is NULL");
    if (cfg->n_init < 1) return capi_fail(DSP_EINVAL, "dsp_kmeans_ubm_config: n_init must be >= 1, got " + std::to_string(cfg->n_init));
    if (const int rc = check_kmeans_numbers(cfg->kmeans_max_iter, cfg->kmeans_tol, cfg->em.reg_covar, "dsp_kmeans_ubm_config: kmeans_")) return rc;
    if (cfg->em.max_iter < 1) return capi_fail(DSP_EINVAL, "dsp_kmeans_ubm_config: em.max_iter must be >= 1, got " + std::to_string(cfg->em.max_iter));
    if (!(cfg->em.tol >= 0.0)) return capi_fail(DSP_EINVAL, "dsp_kmeans_ubm_config: em.tol must be >= 0");
    if (const int rc = check_ubm_result(result)) return rc;
    if (!report || !report->restarts) return capi_fail(DSP_EINVAL, "dsp_kmeans_ubm_report and its restarts must not be NULL");
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t s = (hipStream_t)stream;
    const int k = t->k, d = t->d;
    const size_t kd = (size_t)k * d;
    double limit = 0.0;
    if (const int rc = shift_limit_of(t, d_feats, n, cfg->kmeans_tol, &limit, s)) return rc;
    // everything both halves need, before the first of them: the GMM start must survive in the workspace from Lloyd's final pass to EM
    if (const int rc = reserve_kmeans(t, n, cfg->em.max_iter, true)) return rc;
    std::vector<double> params(dsp::ubm_param_doubles(k, d)), best_params, bounds((size_t)cfg->em.max_iter), best_bounds, centres0(kd);
    std::vector<float> picked(kd);
    int best = -1, best_iter = 0, best_converged = 0;
    for (int r = 0; r < cfg->n_init; ++r) {
        dsp_kmeans_restart &rep = report->restarts[r];
        if (const int rc = seed_rows(t, d_feats, n, dsp::kmeans_restart_seed(cfg->seed, r), rep.rows, s)) return rc;
        for (int i = 0; i < k; ++i)
            DSP_CAPI_HIP(hipMemcpyAsync(picked.data() + (size_t)i * d, d_feats + (size_t)rep.rows[i] * d, (size_t)d * sizeof(float), hipMemcpyDeviceToHost, s));
        DSP_CAPI_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i < kd; ++i) centres0[i] = (double)picked[i];
        dsp::KmeansCtrl end{};
        if (const int rc = run_lloyd(t, d_feats, n, centres0.data(), cfg->kmeans_max_iter, limit, cfg->em.reg_covar, nullptr, &end, s)) return rc;
        int n_iter = 0, converged = 0;
        if (const int rc = run_em_from_device(t, k, d_feats, n, cfg->em.max_iter, cfg->em.tol, cfg->em.reg_covar, params.data(), bounds.data(), &n_iter, &converged, s))
            return rc;
        rep.kmeans_n_iter = end.n_iter;
        rep.kmeans_stop = end.reason;
        rep.kmeans_n_empty = end.n_empty;
        rep.em_n_iter = n_iter;
        rep.em_converged = converged;
        rep.lower_bound = bounds[(size_t)n_iter - 1];
        if (best < 0 || rep.lower_bound > report->restarts[best].lower_bound) {      // ties to the first
            best = r;
            best_params = params;
            best_bounds.assign(bounds.begin(), bounds.begin() + n_iter);
            best_iter = n_iter;
            best_converged = converged;
        }
    }
    for (int i = 0; i < best_iter; ++i) result->lower_bounds[i] = best_bounds[(size_t)i];
    write_ubm_result(result, k, d, best_params, best_iter, best_converged);
    report->winner = best;
    return DSP_OK;
}

int dsp_gmm_quantize(const dsp_gmm_float_params *g, int8_t *means, int32_t *inv_covs, int16_t *log_consts, int saturated[3])
{
    if (const int rc = dsp::check_gmm_float_params(g, "the float GMM", "")) return rc;
    if (!means || !inv_covs || !log_consts || !saturated) return capi_fail(DSP_EINVAL, "means, inv_covs, log_consts and saturated must not be NULL");
    const size_t kd = (size_t)g->k * g->d;
    for (size_t i = 0; i < kd; ++i)
        if (std::isnan(g->means[i]) || std::isnan(g->inv_covs[i])) return capi_fail(DSP_EINVAL, "means and inv_covs must not be NaN");
    for (int i = 0; i < g->k; ++i)
        if (std::isnan(g->log_consts[i])) return capi_fail(DSP_EINVAL, "log_consts must not be NaN");
    // rint: to nearest, ties to even (the default rounding mode); each table saturates to its type and counts what it clamped
    auto quantise = [](double v, double scale, double lo, double hi, int &clamped) {
        const double q = std::rint(v * scale);
        clamped += q < lo || q > hi;
        return q < lo ? lo : q > hi ? hi : q;
    };
    saturated[0] = saturated[1] = saturated[2] = 0;
    for (size_t i = 0; i < kd; ++i) {
        means[i] = (int8_t)quantise(g->means[i], 64.0, -128.0, 127.0, saturated[0]);
        inv_covs[i] = (int32_t)quantise(g->inv_covs[i], 2048.0, -2147483648.0, 2147483647.0, saturated[1]);
    }
    for (int i = 0; i < g->k; ++i) log_consts[i] = (int16_t)quantise(g->log_consts[i], 256.0, -32768.0, 32767.0, saturated[2]);
    return DSP_OK;
}

}  // extern "C"
