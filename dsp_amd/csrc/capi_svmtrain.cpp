// capi_svmtrain.cpp -- the C ABI of SVM training (include/dsp_amd.h dsp_svm_train_*, dsp_svm_fit_device): argument
// checks, all of them before a device is touched, the host helpers (folds, balanced weights, model compaction), the trainer's grow-only
// workspace and the problem tables that travel through its ring to the kernels of svmtrain_kernels.hip.
#include <cmath>
#include <cstdint>
#include <memory>

#include "capi_util.hpp"
#include "kmeans_kernels.hpp"
#include "svmtrain_kernels.hpp"

using dsp::capi_fail;

static_assert(sizeof(dsp_svm_train_result) == 40, "dsp_svm_train_result is 40 bytes (dsp_amd/lib.py SvmTrainResult)");
static_assert(sizeof(dsp_svm_train_problem) == 40, "dsp_svm_train_problem is 40 bytes (dsp_amd/lib.py SvmTrainProblem)");
static_assert(sizeof(dsp_svm_train_config) == 16, "dsp_svm_train_config is 16 bytes (dsp_amd/lib.py SvmTrainConfig)");
static_assert(sizeof(dsp_svm_fit_model) == 112, "dsp_svm_fit_model is 112 bytes (dsp_amd/lib.py SvmFitModel)");
static_assert(DSP_SVM_TRAIN_MAX_ROWS == dsp::kSvmTrainMaxRows, "the header's cap is the kernels'");

struct dsp_svm_trainer : dsp::Handle {
    int n_features = 0;
    long n = 0;                                    // rows of the current dataset, 0: none
    dsp::DeviceBuf<float> scaler, z;               // offset | scale; z[n][nf]
    dsp::DeviceBuf<double> d2;                     // [n][n]
    dsp::DeviceBuf<char> table;                    // dsp_svm_train_result[P] of the last launch
    dsp::DeviceBuf<double> fit;                    // dsp_svm_fit_device: coef[k + 1][n] | dec[k + 1][n] | dec_cv[n]
    dsp::SpanRing spans;
};

namespace {

int check_trainer(const dsp_svm_trainer *t) { return t ? DSP_OK : capi_fail(DSP_EINVAL, "trainer is NULL"); }

int check_rows(long n)
{
    if (n < 2) return capi_fail(DSP_EINVAL, "n must be >= 2, got " + std::to_string(n));
    if (n > dsp::kSvmTrainMaxRows) return capi_fail(DSP_EINVAL, "n = " + std::to_string(n) + " is above the cap of 8192 rows (DSP_SVM_TRAIN_MAX_ROWS)");
    return DSP_OK;
}

int check_labels(const int *labels, long n)
{
    if (!labels) return capi_fail(DSP_EINVAL, "labels is NULL");
    for (long r = 0; r < n; ++r)
        if (labels[r] != 0 && labels[r] != 1) return capi_fail(DSP_EINVAL, "labels[" + std::to_string(r) + "] = " + std::to_string(labels[r]) + " is neither 0 nor 1");
    return DSP_OK;
}

int check_config(const dsp_svm_train_config *cfg, double &eps, int &max_iter, int &q_float32)
{
    q_float32 = cfg ? cfg->q_float32 : 0;
    if (q_float32 != 0 && q_float32 != 1) return capi_fail(DSP_EINVAL, "dsp_svm_train_config: q_float32 must be 0 or 1, got " + std::to_string(q_float32));
    eps = cfg ? cfg->eps : 1e-3;
    max_iter = cfg && cfg->max_iter ? cfg->max_iter : dsp::kSvmTrainDefaultIter;
    if (!(std::isfinite(eps) && eps > 0.0)) return capi_fail(DSP_EINVAL, "dsp_svm_train_config: eps must be finite and > 0");
    if (max_iter < 0 || max_iter > dsp::kSvmTrainMaxIter)
        return capi_fail(DSP_EINVAL, "dsp_svm_train_config: max_iter must be 0 .. 100000000, got " + std::to_string(max_iter));
    return DSP_OK;
}

int check_box(double c0, double c1, double gamma, const std::string &who)
{
    if (!(std::isfinite(c0) && c0 > 0.0)) return capi_fail(DSP_EINVAL, who + "c_label0 must be finite and > 0");
    if (!(std::isfinite(c1) && c1 > 0.0)) return capi_fail(DSP_EINVAL, who + "c_label1 must be finite and > 0");
    if (!(std::isfinite(gamma) && gamma >= 0.0)) return capi_fail(DSP_EINVAL, who + "gamma must be finite and >= 0");
    return DSP_OK;
}

int check_problems(const dsp_svm_train_problem *problems, long n_problems, long n, size_t &total, int &max_members)
{
    total = 0;
    max_members = 0;
    for (long p = 0; p < n_problems; ++p) {
        const dsp_svm_train_problem &pr = problems[p];
        const std::string who = "problems[" + std::to_string(p) + "]: ";
        if (pr.n_rows < 0 || pr.n_rows > n) return capi_fail(DSP_EINVAL, who + "n_rows must be 0 .. n");
        if (pr.n_rows && !pr.rows) return capi_fail(DSP_EINVAL, who + "rows is NULL");
        if (const int rc = check_box(pr.c_label0, pr.c_label1, pr.gamma, who)) return rc;
        for (long k = 0; k < pr.n_rows; ++k) {
            if (pr.rows[k] < 0 || pr.rows[k] >= n) return capi_fail(DSP_EINVAL, who + "rows[" + std::to_string(k) + "] = " + std::to_string(pr.rows[k]) + " is out of range");
            if (k && pr.rows[k] <= pr.rows[k - 1]) return capi_fail(DSP_EINVAL, who + "rows must be strictly ascending (rows[" + std::to_string(k) + "])");
        }
        total += (size_t)pr.n_rows;
        max_members = std::max(max_members, (int)pr.n_rows);
    }
    return DSP_OK;
}

// The problems' table, the labels and the member lists through the ring, the solver and the decision pass: enqueued, not waited for.
// d_results (in the trainer's table) holds the results afterwards.
int enqueue_problems(dsp_svm_trainer *t, const dsp_svm_train_problem *problems, long n_problems, size_t total, int max_members, double eps,
                     int max_iter, int q_float32, const int *labels, double *d_coef, double *d_dec, const dsp_svm_train_result *&d_results, hipStream_t st)
{
    const size_t n = (size_t)t->n, P = (size_t)n_problems;
    const size_t bytes = P * sizeof(dsp::SvmTrainProblem) + (n + total) * sizeof(int);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(t->spans, bytes, slot)) return rc;
    auto *h_prob = static_cast<dsp::SvmTrainProblem *>(slot.h());
    int *h_labels = reinterpret_cast<int *>(h_prob + P), *h_members = h_labels + n;
    std::memcpy(h_labels, labels, n * sizeof(int));
    size_t first = 0;
    for (size_t p = 0; p < P; ++p) {
        const dsp_svm_train_problem &pr = problems[p];
        long n0 = 0;
        for (long k = 0; k < pr.n_rows; ++k) {
            h_members[first + (size_t)k] = pr.rows[k];
            n0 += labels[pr.rows[k]] == 0;
        }
        int status = DSP_SVM_TRAIN_CONVERGED;
        double fill = 0.0;
        if (pr.n_rows == 0) status = DSP_SVM_TRAIN_EMPTY;
        else if (n0 == pr.n_rows || n0 == 0) { status = DSP_SVM_TRAIN_ONE_CLASS; fill = n0 ? 1.0 : -1.0; }
        h_prob[p] = dsp::SvmTrainProblem{(long)first, (int)pr.n_rows, status, {pr.c_label0, pr.c_label1}, pr.gamma, fill};
        first += (size_t)pr.n_rows;
    }
    if (t->table.reserve(P * sizeof(dsp_svm_train_result)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the trainer's result table");
    DSP_CAPI_HIP(slot.upload(bytes, st));
    const auto *d_prob = static_cast<const dsp::SvmTrainProblem *>(slot.d());
    const int *d_labels = reinterpret_cast<const int *>(d_prob + P), *d_members = d_labels + n;
    auto *res = reinterpret_cast<dsp_svm_train_result *>(t->table.get());
    DSP_CAPI_HIP(hipMemsetAsync(d_coef, 0, P * n * sizeof(double), st));
    DSP_CAPI_HIP(dsp::launch_svm_smo(t->d2, t->n, d_members, d_prob, n_problems, max_members, d_labels, eps, max_iter, q_float32, d_coef, res, st));
    if (d_dec) DSP_CAPI_HIP(dsp::launch_svm_decisions(t->d2, t->n, d_members, d_prob, n_problems, d_coef, res, d_dec, st));
    d_results = res;
    return DSP_OK;
}

int enqueue_platt(dsp_svm_trainer *t, const double *d_dec_cv, const int *labels, const int *rows, long n_rows, dsp::SvmPlattOut *&d_out, hipStream_t st)
{
    const size_t n = (size_t)t->n, bytes = (n + (rows ? (size_t)n_rows : 0)) * sizeof(int);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(t->spans, bytes, slot)) return rc;
    int *h = static_cast<int *>(slot.h());
    std::memcpy(h, labels, n * sizeof(int));
    if (rows) std::memcpy(h + n, rows, (size_t)n_rows * sizeof(int));
    DSP_CAPI_HIP(slot.upload(bytes, st));
    const int *d = static_cast<const int *>(slot.d());
    // (behind the Scaler, in the buffer a dataset reserves: enqueue_dataset)
    d_out = reinterpret_cast<dsp::SvmPlattOut *>(reinterpret_cast<char *>(t->scaler.get()) + (2 * (size_t)t->n_features * sizeof(float) + 15) / 16 * 16);
    DSP_CAPI_HIP(dsp::launch_svm_platt(d_dec_cv, d, rows ? d + n : nullptr, rows ? n_rows : t->n, d_out, st));
    return DSP_OK;
}

// the Scaler (fitted or the caller's), z and D2 of a new dataset: enqueued
int enqueue_dataset(dsp_svm_trainer *t, const float *d_feat, long n, const int *scaler_rows, long n_scaler_rows, const float *offset,
                    const float *scale, hipStream_t st)
{
    const size_t nf = (size_t)t->n_features;
    t->n = 0;
    // (the Scaler's buffer also holds the Platt fit's output behind it: enqueue_platt)
    if (t->scaler.reserve(2 * nf * sizeof(float) + sizeof(dsp::SvmPlattOut) + 16) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the trainer's Scaler");
    if (t->z.reserve((size_t)n * nf * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the standardised rows");
    if (t->d2.reserve((size_t)n * (size_t)n * sizeof(double)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the distance matrix");
    float *d_offset = t->scaler, *d_scale = t->scaler.get() + nf;
    if (offset) {
        const size_t bytes = 2 * nf * sizeof(float);
        dsp::SpanRing::Lease slot;
        if (const int rc = dsp::lease(t->spans, bytes, slot)) return rc;
        std::memcpy(slot.h(), offset, nf * sizeof(float));
        std::memcpy(static_cast<float *>(slot.h()) + nf, scale, nf * sizeof(float));
        DSP_CAPI_HIP(slot.upload(bytes, st));
        DSP_CAPI_HIP(hipMemcpyAsync(d_offset, slot.d(), bytes, hipMemcpyDeviceToDevice, st));
    } else if (scaler_rows) {
        const size_t bytes = (size_t)n_scaler_rows * sizeof(int);
        dsp::SpanRing::Lease slot;
        if (const int rc = dsp::lease(t->spans, bytes, slot)) return rc;
        std::memcpy(slot.h(), scaler_rows, bytes);
        DSP_CAPI_HIP(slot.upload(bytes, st));
        DSP_CAPI_HIP(dsp::launch_svm_scaler_fit(d_feat, t->n_features, static_cast<const int *>(slot.d()), n_scaler_rows, d_offset, d_scale, st));
    } else {
        DSP_CAPI_HIP(dsp::launch_svm_scaler_fit(d_feat, t->n_features, nullptr, n, d_offset, d_scale, st));
    }
    DSP_CAPI_HIP(dsp::launch_svm_distances(d_feat, n, t->n_features, d_offset, d_scale, t->z, t->d2, st));
    t->n = n;
    return DSP_OK;
}

long compact_model(const float *z, const int *labels, const double *coef, long n, int n_features, float *sv, float *coef_out, long capacity,
                   long *n_sv_label0)
{
    long count = 0;
    for (int label = 0; label < 2; ++label) {
        for (long r = 0; r < n; ++r) {
            if (labels[r] != label || coef[r] == 0.0) continue;
            if (sv && coef_out) {
                if (count >= capacity) return capi_fail(DSP_EINVAL, "more support vectors than capacity = " + std::to_string(capacity));
                std::memcpy(sv + (size_t)count * n_features, z + (size_t)r * n_features, (size_t)n_features * sizeof(float));
                coef_out[count] = (float)coef[r];
            }
            ++count;
        }
        if (label == 0 && n_sv_label0) *n_sv_label0 = count;
    }
    return count;
}

void make_folds(long n, int k, uint64_t seed, int *fold_ids)
{
    std::vector<long> perm((size_t)n);
    for (long i = 0; i < n; ++i) perm[(size_t)i] = i;
    for (long i = 0; i < n; ++i) {
        const long j = i + (long)(dsp::kmeans_mix(seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull) % (uint64_t)(n - i));
        std::swap(perm[(size_t)i], perm[(size_t)j]);
    }
    for (int f = 0; f < k; ++f)
        for (long p = (long)f * n / k; p < (long)(f + 1) * n / k; ++p) fold_ids[perm[(size_t)p]] = f;
}

}  // namespace

extern "C" {

int dsp_svm_trainer_create(int device, int n_features, dsp_svm_trainer **out)
{
    // no device is touched here: a device that does not exist is reported by the first call that takes a dataset
    return dsp::create_on_host(device, out, [&](dsp_svm_trainer &t) -> int {
        if (n_features < 1) return capi_fail(DSP_EINVAL, "n_features must be >= 1, got " + std::to_string(n_features));
        t.n_features = n_features;
        return DSP_OK;
    });
}

void dsp_svm_trainer_destroy(dsp_svm_trainer *t) { dsp::destroy(t); }

int dsp_svm_train_set_device(dsp_svm_trainer *t, const float *d_feat, long n, const int *scaler_rows, long n_scaler_rows, const float *offset,
                             const float *scale, float *offset_out, float *scale_out, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (!d_feat) return capi_fail(DSP_EINVAL, "d_feat is NULL");
    if (const int rc = check_rows(n)) return rc;
    if (!offset != !scale) return capi_fail(DSP_EINVAL, "offset and scale must be given together");
    if (offset) {
        for (int f = 0; f < t->n_features; ++f)
            if (!std::isfinite(offset[f]) || !std::isfinite(scale[f])) return capi_fail(DSP_EINVAL, "offset / scale of feature " + std::to_string(f) + " is not finite");
    } else if (scaler_rows) {
        if (n_scaler_rows < 1) return capi_fail(DSP_EINVAL, "n_scaler_rows must be >= 1");
        for (long k = 0; k < n_scaler_rows; ++k)
            if (scaler_rows[k] < 0 || scaler_rows[k] >= n)
                return capi_fail(DSP_EINVAL, "scaler_rows[" + std::to_string(k) + "] = " + std::to_string(scaler_rows[k]) + " is out of range");
    }
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = enqueue_dataset(t, d_feat, n, scaler_rows, n_scaler_rows, offset, scale, st)) return rc;
    if (offset_out || scale_out) {
        const size_t nf = (size_t)t->n_features;
        if (offset_out) DSP_CAPI_HIP(hipMemcpyAsync(offset_out, t->scaler.get(), nf * sizeof(float), hipMemcpyDeviceToHost, st));
        if (scale_out) DSP_CAPI_HIP(hipMemcpyAsync(scale_out, t->scaler.get() + nf, nf * sizeof(float), hipMemcpyDeviceToHost, st));
        DSP_CAPI_HIP(hipStreamSynchronize(st));
    }
    return DSP_OK;
}

int dsp_svm_train_rows_host(dsp_svm_trainer *t, float *z, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (!z) return capi_fail(DSP_EINVAL, "z is NULL");
    if (t->n == 0) return capi_fail(DSP_EINVAL, "the trainer has no dataset (dsp_svm_train_set_device)");
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    DSP_CAPI_HIP(hipMemcpyAsync(z, t->z.get(), (size_t)t->n * (size_t)t->n_features * sizeof(float), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    return DSP_OK;
}

int dsp_svm_train_problems_device(dsp_svm_trainer *t, const dsp_svm_train_problem *problems, long n_problems, const dsp_svm_train_config *cfg,
                                  const int *labels, dsp_svm_train_result *results, double *d_coef, double *d_dec, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (n_problems < 0 || n_problems > INT32_MAX) return capi_fail(DSP_EINVAL, "n_problems must be 0 .. 2^31 - 1");
    double eps;
    int max_iter, q_float32;
    if (const int rc = check_config(cfg, eps, max_iter, q_float32)) return rc;
    if (t->n == 0) return capi_fail(DSP_EINVAL, "the trainer has no dataset (dsp_svm_train_set_device)");
    if (n_problems == 0) return DSP_OK;
    if (!problems) return capi_fail(DSP_EINVAL, "problems is NULL");
    if (!results) return capi_fail(DSP_EINVAL, "results is NULL");
    if (!d_coef) return capi_fail(DSP_EINVAL, "d_coef is NULL");
    if (const int rc = check_labels(labels, t->n)) return rc;
    size_t total;
    int max_members;
    if (const int rc = check_problems(problems, n_problems, t->n, total, max_members)) return rc;
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    const dsp_svm_train_result *d_results = nullptr;
    if (const int rc = enqueue_problems(t, problems, n_problems, total, max_members, eps, max_iter, q_float32, labels, d_coef, d_dec, d_results, st)) return rc;
    DSP_CAPI_HIP(hipMemcpyAsync(results, d_results, (size_t)n_problems * sizeof(*results), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    return DSP_OK;
}

int dsp_svm_platt_fit_device(dsp_svm_trainer *t, const double *d_dec_cv, const int *labels, const int *rows, long n_rows, double *a, double *b,
                             int *n_iter, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (!d_dec_cv) return capi_fail(DSP_EINVAL, "d_dec_cv is NULL");
    if (!a || !b) return capi_fail(DSP_EINVAL, "a and b must not be NULL");
    if (t->n == 0) return capi_fail(DSP_EINVAL, "the trainer has no dataset (dsp_svm_train_set_device)");
    if (const int rc = check_labels(labels, t->n)) return rc;
    if (rows) {
        if (n_rows < 1) return capi_fail(DSP_EINVAL, "n_rows must be >= 1");
        for (long k = 0; k < n_rows; ++k)
            if (rows[k] < 0 || rows[k] >= t->n) return capi_fail(DSP_EINVAL, "rows[" + std::to_string(k) + "] = " + std::to_string(rows[k]) + " is out of range");
    }
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    dsp::SvmPlattOut *d_out = nullptr, out;
    if (const int rc = enqueue_platt(t, d_dec_cv, labels, rows, n_rows, d_out, st)) return rc;
    DSP_CAPI_HIP(hipMemcpyAsync(&out, d_out, sizeof(out), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    *a = out.a;
    *b = out.b;
    if (n_iter) *n_iter = out.n_iter;
    return DSP_OK;
}

int dsp_svm_folds(long n, int k, unsigned long long seed, int *fold_ids)
{
    if (!fold_ids) return capi_fail(DSP_EINVAL, "fold_ids is NULL");
    if (n < 1) return capi_fail(DSP_EINVAL, "n must be >= 1");
    if (k < 1 || k > n) return capi_fail(DSP_EINVAL, "k must be 1 .. n, got " + std::to_string(k));
    make_folds(n, k, seed, fold_ids);
    return DSP_OK;
}

int dsp_svm_balanced_weights(const int *labels, const int *rows, long n_rows, double c, double *c_label0, double *c_label1)
{
    if (!labels || !c_label0 || !c_label1) return capi_fail(DSP_EINVAL, "labels, c_label0 and c_label1 must not be NULL");
    if (n_rows < 1) return capi_fail(DSP_EINVAL, "n_rows must be >= 1");
    if (!(std::isfinite(c) && c > 0.0)) return capi_fail(DSP_EINVAL, "c must be finite and > 0");
    long count[2] = {0, 0};
    for (long k = 0; k < n_rows; ++k) {
        if (rows && rows[k] < 0) return capi_fail(DSP_EINVAL, "rows[" + std::to_string(k) + "] is negative");
        const int label = labels[rows ? rows[k] : k];
        if (label != 0 && label != 1) return capi_fail(DSP_EINVAL, "the label of row " + std::to_string(rows ? rows[k] : k) + " is neither 0 nor 1");
        ++count[label];
    }
    if (!count[0] || !count[1]) return capi_fail(DSP_EINVAL, std::string("label ") + (count[0] ? "1" : "0") + " has no row");
    *c_label0 = c * (double)n_rows / (2.0 * (double)count[0]);
    *c_label1 = c * (double)n_rows / (2.0 * (double)count[1]);
    return DSP_OK;
}

long dsp_svm_model_from_training(const float *z, const int *labels, const double *coef, long n, int n_features, float *sv, float *coef_out,
                                 long capacity, long *n_sv_label0)
{
    if (!z || !coef) return capi_fail(DSP_EINVAL, "z and coef must not be NULL");
    if (n < 1) return capi_fail(DSP_EINVAL, "n must be >= 1");
    if (n_features < 1) return capi_fail(DSP_EINVAL, "n_features must be >= 1");
    if (const int rc = check_labels(labels, n)) return rc;
    return compact_model(z, labels, coef, n, n_features, sv, coef_out, capacity, n_sv_label0);
}

int dsp_svm_fit_device(dsp_svm_trainer *t, const float *d_feat, long n, const int *labels, const int *fold_ids, int k_prob,
                       unsigned long long seed, double c_label0, double c_label1, double gamma, const dsp_svm_train_config *cfg,
                       dsp_svm_fit_model *model, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (!d_feat) return capi_fail(DSP_EINVAL, "d_feat is NULL");
    if (const int rc = check_rows(n)) return rc;
    if (const int rc = check_labels(labels, n)) return rc;
    if (k_prob < 2 || k_prob > 64 || k_prob > n) return capi_fail(DSP_EINVAL, "k_prob must be 2 .. min(64, n), got " + std::to_string(k_prob));
    if (fold_ids)
        for (long r = 0; r < n; ++r)
            if (fold_ids[r] < 0 || fold_ids[r] >= k_prob)
                return capi_fail(DSP_EINVAL, "fold_ids[" + std::to_string(r) + "] = " + std::to_string(fold_ids[r]) + " is outside 0 .. k_prob - 1");
    if (const int rc = check_box(c_label0, c_label1, gamma, "")) return rc;
    double eps;
    int max_iter, q_float32;
    if (const int rc = check_config(cfg, eps, max_iter, q_float32)) return rc;
    if (!model || !model->offset || !model->scale || !model->sv || !model->coef) return capi_fail(DSP_EINVAL, "model and its arrays must not be NULL");
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    gamma = (double)(float)gamma;                  // the model's gamma is a float: the fit trains with the value the model will hold
    // the k_prob problems without one fold each, then the problem on all rows
    std::vector<int> folds((size_t)n);
    if (fold_ids) std::memcpy(folds.data(), fold_ids, (size_t)n * sizeof(int)); else make_folds(n, k_prob, seed, folds.data());
    const long P = k_prob + 1;
    std::vector<std::vector<int>> rows((size_t)P);
    std::vector<dsp_svm_train_problem> problems((size_t)P);
    for (long p = 0; p < P; ++p) {
        for (long r = 0; r < n; ++r)
            if (p == k_prob || folds[(size_t)r] != p) rows[(size_t)p].push_back((int)r);
        problems[(size_t)p] = dsp_svm_train_problem{rows[(size_t)p].data(), (long)rows[(size_t)p].size(), c_label0, c_label1, gamma};
    }
    size_t total;
    int max_members;
    if (const int rc = check_problems(problems.data(), P, n, total, max_members)) return rc;
    if (const int rc = enqueue_dataset(t, d_feat, n, nullptr, 0, nullptr, nullptr, st)) return rc;
    const size_t un = (size_t)n;
    // coef[P][n] | dec[P][n] | dec_cv[n], then the fold ids as ints
    if (t->fit.reserve(((size_t)(2 * P + 1) * un) * sizeof(double) + un * sizeof(int)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the fit's workspace");
    double *d_coef = t->fit, *d_dec = d_coef + (size_t)P * un, *d_cv = d_dec + (size_t)P * un;
    int *d_folds = reinterpret_cast<int *>(d_cv + un);
    const dsp_svm_train_result *d_results = nullptr;
    if (const int rc = enqueue_problems(t, problems.data(), P, total, max_members, eps, max_iter, q_float32, labels, d_coef, d_dec, d_results, st)) return rc;
    DSP_CAPI_HIP(hipMemcpyAsync(d_folds, folds.data(), un * sizeof(int), hipMemcpyHostToDevice, st));
    DSP_CAPI_HIP(dsp::launch_svm_gather_cv(d_dec, n, d_folds, d_cv, st));
    dsp::SvmPlattOut *d_platt = nullptr, platt;
    if (const int rc = enqueue_platt(t, d_cv, labels, nullptr, 0, d_platt, st)) return rc;
    const size_t nf = (size_t)t->n_features;
    std::vector<double> coef(un);
    std::vector<float> z(un * nf);
    DSP_CAPI_HIP(hipMemcpyAsync(&model->final, d_results + k_prob, sizeof(model->final), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipMemcpyAsync(&platt, d_platt, sizeof(platt), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipMemcpyAsync(coef.data(), d_coef + (size_t)k_prob * un, un * sizeof(double), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipMemcpyAsync(z.data(), t->z.get(), un * nf * sizeof(float), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipMemcpyAsync(model->offset, t->scaler.get(), nf * sizeof(float), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipMemcpyAsync(model->scale, t->scaler.get() + nf, nf * sizeof(float), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    model->n_sv = compact_model(z.data(), labels, coef.data(), n, t->n_features, model->sv, model->coef, n, &model->n_sv_label0);
    model->rho = (float)model->final.rho;
    model->prob_a = (float)platt.a;
    model->prob_b = (float)platt.b;
    model->gamma = (float)gamma;
    model->platt_iter = platt.n_iter;
    model->reserved = 0;
    return DSP_OK;
}

}  // extern "C"
