// capi_stoptrain.cpp -- the C ABI of stop-net training (include/dsp_amd.h dsp_stop_train_*): argument checks, all of
// them before a device is touched, the host helpers (the library's draws, the epoch order, the initial weights, the float32 model of a
// trained net), the trainer's grow-only workspace and the run tables that travel through its ring to the kernels of
// stoptrain_kernels.hip.
#include <cmath>
#include <cstdint>
#include <memory>

#include "capi_util.hpp"
#include "stoptrain_kernels.hpp"

using dsp::capi_fail;

static_assert(sizeof(dsp_stop_train_run) == 88, "dsp_stop_train_run is 88 bytes (dsp_amd/lib.py StopTrainRun)");
static_assert(sizeof(dsp_stop_train_result) == 40, "dsp_stop_train_result is 40 bytes (dsp_amd/lib.py StopTrainResult)");
static_assert(DSP_STOP_TRAIN_CAP_ROWS == dsp::kStopTrainMaxRows && DSP_STOP_TRAIN_CAP_UNITS == dsp::kStopTrainMaxUnits &&
              DSP_STOP_TRAIN_CAP_BATCH == dsp::kStopTrainMaxBatch && DSP_STOP_TRAIN_CAP_EPOCHS == dsp::kStopTrainMaxEpochs &&
              DSP_STOP_TRAIN_CAP_RUNS == dsp::kStopTrainMaxRuns, "the header's caps are the kernels'");

struct dsp_stop_trainer : dsp::Handle {
    int n_coef = 0, max_frames = 0, units[4] = {0, 0, 0, 0};
    long n = 0;                                    // clips of the current dataset, 0: none
    dsp::StopTrainShape shape{};                   // of the current dataset (t_used, f_used)
    dsp::DeviceBuf<float> scaler, z;               // mean | scale over all inputs; z[n][f_used]
    dsp::DeviceBuf<long> offsets;                  // frame_offsets[n + 1]
    dsp::DeviceBuf<double> slabs;                  // the launch's runs: kernel1, moments, snapshot
    dsp::DeviceBuf<char> table;                    // StopTrainState[P] | dsp_stop_train_result[P] | stop[P]
    dsp::SpanRing spans;
};

namespace {

int check_trainer(const dsp_stop_trainer *t) { return t ? DSP_OK : capi_fail(DSP_EINVAL, "trainer is NULL"); }

int check_shape(int n_coef, int max_frames, const int *units)
{
    if (n_coef < 1) return capi_fail(DSP_EINVAL, "n_coef must be >= 1, got " + std::to_string(n_coef));
    if (max_frames < 1) return capi_fail(DSP_EINVAL, "max_frames must be >= 1, got " + std::to_string(max_frames));
    if ((long)n_coef * max_frames > INT32_MAX / dsp::kStopTrainMaxUnits) return capi_fail(DSP_EINVAL, "n_coef * max_frames is too large");
    if (!units) return capi_fail(DSP_EINVAL, "units is NULL");
    for (int l = 0; l < 4; ++l)
        if (units[l] < 1 || units[l] > dsp::kStopTrainMaxUnits)
            return capi_fail(DSP_EINVAL, "units[" + std::to_string(l) + "] must be 1 .. 16 (DSP_STOP_TRAIN_CAP_UNITS), got " + std::to_string(units[l]));
    if (units[3] != 1) return capi_fail(DSP_EINVAL, "units[3] must be 1 (sigmoid output)");
    return DSP_OK;
}

int check_labels(const int *labels, long n)
{
    if (!labels) return capi_fail(DSP_EINVAL, "labels is NULL");
    for (long r = 0; r < n; ++r)
        if (labels[r] != 0 && labels[r] != 1) return capi_fail(DSP_EINVAL, "labels[" + std::to_string(r) + "] = " + std::to_string(labels[r]) + " is neither 0 nor 1");
    return DSP_OK;
}

int check_row_list(const int *rows, long n_rows, long n, const std::string &who, const char *name)
{
    if (n_rows < 0 || n_rows > n) return capi_fail(DSP_EINVAL, who + "n_" + (name + std::string(" must be 0 .. n")));
    if (n_rows && !rows) return capi_fail(DSP_EINVAL, who + name + "_rows is NULL");
    for (long k = 0; k < n_rows; ++k) {
        if (rows[k] < 0 || rows[k] >= n) return capi_fail(DSP_EINVAL, who + name + "_rows[" + std::to_string(k) + "] = " + std::to_string(rows[k]) + " is out of range");
        if (k && rows[k] <= rows[k - 1]) return capi_fail(DSP_EINVAL, who + name + "_rows must be strictly ascending (" + name + "_rows[" + std::to_string(k) + "])");
    }
    return DSP_OK;
}

// what a run asks for that no dataset is needed to judge
int check_hyper(const dsp_stop_train_run *runs, long n_runs, int &max_epochs)
{
    max_epochs = 0;
    for (long p = 0; p < n_runs; ++p) {
        const dsp_stop_train_run &r = runs[p];
        const std::string who = "runs[" + std::to_string(p) + "]: ";
        if (!(std::isfinite(r.learning_rate) && r.learning_rate > 0.0)) return capi_fail(DSP_EINVAL, who + "learning_rate must be finite and > 0");
        for (int l = 0; l < 3; ++l)
            if (!(r.dropout[l] >= 0.0 && r.dropout[l] < 1.0)) return capi_fail(DSP_EINVAL, who + "dropout[" + std::to_string(l) + "] must be in [0, 1)");
        if (r.batch_size < 1 || r.batch_size > dsp::kStopTrainMaxBatch)
            return capi_fail(DSP_EINVAL, who + "batch_size must be 1 .. 256 (DSP_STOP_TRAIN_CAP_BATCH), got " + std::to_string(r.batch_size));
        if (r.epochs < 1 || r.epochs > dsp::kStopTrainMaxEpochs)
            return capi_fail(DSP_EINVAL, who + "epochs must be 1 .. 10000 (DSP_STOP_TRAIN_CAP_EPOCHS), got " + std::to_string(r.epochs));
        if (r.patience < 0) return capi_fail(DSP_EINVAL, who + "patience must be >= 0, got " + std::to_string(r.patience));
        if (r.restore_best != 0 && r.restore_best != 1) return capi_fail(DSP_EINVAL, who + "restore_best must be 0 or 1, got " + std::to_string(r.restore_best));
        max_epochs = std::max(max_epochs, r.epochs);
    }
    return DSP_OK;
}

int check_run_rows(const dsp_stop_train_run *runs, long n_runs, long n, size_t &total)
{
    total = 0;
    for (long p = 0; p < n_runs; ++p) {
        const dsp_stop_train_run &r = runs[p];
        const std::string who = "runs[" + std::to_string(p) + "]: ";
        if (const int rc = check_row_list(r.train_rows, r.n_train, n, who, "train")) return rc;
        if (const int rc = check_row_list(r.val_rows, r.n_val, n, who, "val")) return rc;
        total += (size_t)r.n_train + (size_t)r.n_val;
    }
    return DSP_OK;
}

}  // namespace

extern "C" {

int dsp_stop_trainer_create(int device, int n_coef, int max_frames, const int *units, dsp_stop_trainer **out)
{
    // no device is touched here: a device that does not exist is reported by the first call that takes a dataset
    return dsp::create_on_host(device, out, [&](dsp_stop_trainer &t) -> int {
        if (const int rc = check_shape(n_coef, max_frames, units)) return rc;
        t.n_coef = n_coef;
        t.max_frames = max_frames;
        std::memcpy(t.units, units, sizeof(t.units));
        return DSP_OK;
    });
}

void dsp_stop_trainer_destroy(dsp_stop_trainer *t) { dsp::destroy(t); }

int dsp_stop_train_set_device(dsp_stop_trainer *t, const float *d_mfcc, long n, const long *frame_offsets, const int *scaler_rows,
                              long n_scaler_rows, const float *mean, const float *scale, float *mean_out, float *scale_out, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (n < 1) return capi_fail(DSP_EINVAL, "n must be >= 1, got " + std::to_string(n));
    if (n > dsp::kStopTrainMaxRows) return capi_fail(DSP_EINVAL, "n = " + std::to_string(n) + " is above the cap of 65536 clips (DSP_STOP_TRAIN_CAP_ROWS)");
    if (!frame_offsets) return capi_fail(DSP_EINVAL, "frame_offsets is NULL");
    if (const int rc = dsp::check_frame_offsets(frame_offsets, n, "clip")) return rc;
    long longest = 0;
    for (long i = 0; i < n; ++i) longest = std::max(longest, frame_offsets[i + 1] - frame_offsets[i]);
    if (longest > 0 && !d_mfcc) return capi_fail(DSP_EINVAL, "d_mfcc is NULL");
    if (!mean != !scale) return capi_fail(DSP_EINVAL, "mean and scale must be given together");
    const size_t n_in = (size_t)t->n_coef * t->max_frames;
    if (mean) {
        for (size_t j = 0; j < n_in; ++j)
            if (!std::isfinite(mean[j]) || !std::isfinite(scale[j])) return capi_fail(DSP_EINVAL, "mean / scale of feature " + std::to_string(j) + " is not finite");
    } else if (scaler_rows) {
        if (n_scaler_rows < 1) return capi_fail(DSP_EINVAL, "n_scaler_rows must be >= 1");
        for (long k = 0; k < n_scaler_rows; ++k)
            if (scaler_rows[k] < 0 || scaler_rows[k] >= n)
                return capi_fail(DSP_EINVAL, "scaler_rows[" + std::to_string(k) + "] = " + std::to_string(scaler_rows[k]) + " is out of range");
    }
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    t->n = 0;
    const dsp::StopTrainShape s = dsp::stop_train_shape(t->n_coef, t->max_frames, t->units, (int)std::min<long>(t->max_frames, longest));
    if (t->scaler.reserve(2 * n_in * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the trainer's Scaler");
    if (t->z.reserve(std::max<size_t>((size_t)n * s.f_used, 1) * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the standardised rows");
    if (t->offsets.reserve((size_t)(n + 1) * sizeof(long)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the clips' offsets");
    float *d_mean = t->scaler, *d_scale = t->scaler.get() + n_in;
    {
        // offsets[n + 1], then the caller's Scaler or the scaler rows
        const size_t head = (size_t)(n + 1) * sizeof(long);
        const size_t bytes = head + (mean ? 2 * n_in * sizeof(float) : (scaler_rows ? (size_t)n_scaler_rows * sizeof(int) : 0));
        dsp::SpanRing::Lease slot;
        if (const int rc = dsp::lease(t->spans, bytes, slot)) return rc;
        char *h = static_cast<char *>(slot.h());
        std::memcpy(h, frame_offsets, head);
        if (mean) {
            std::memcpy(h + head, mean, n_in * sizeof(float));
            std::memcpy(h + head + n_in * sizeof(float), scale, n_in * sizeof(float));
        } else if (scaler_rows) {
            std::memcpy(h + head, scaler_rows, (size_t)n_scaler_rows * sizeof(int));
        }
        DSP_CAPI_HIP(slot.upload(bytes, st));
        const char *d = static_cast<const char *>(slot.d());
        DSP_CAPI_HIP(hipMemcpyAsync(t->offsets.get(), d, head, hipMemcpyDeviceToDevice, st));
        if (mean) DSP_CAPI_HIP(hipMemcpyAsync(d_mean, d + head, 2 * n_in * sizeof(float), hipMemcpyDeviceToDevice, st));
        else
            DSP_CAPI_HIP(dsp::launch_stop_train_scaler(d_mfcc, t->offsets, s, scaler_rows ? reinterpret_cast<const int *>(d + head) : nullptr,
                                                       scaler_rows ? n_scaler_rows : n, d_mean, d_scale, st));
    }
    if (s.f_used) DSP_CAPI_HIP(dsp::launch_stop_train_standardise(d_mfcc, t->offsets, n, s, d_mean, d_scale, t->z, st));
    t->shape = s;
    t->n = n;
    if (mean_out || scale_out) {
        if (mean_out) DSP_CAPI_HIP(hipMemcpyAsync(mean_out, d_mean, n_in * sizeof(float), hipMemcpyDeviceToHost, st));
        if (scale_out) DSP_CAPI_HIP(hipMemcpyAsync(scale_out, d_scale, n_in * sizeof(float), hipMemcpyDeviceToHost, st));
        DSP_CAPI_HIP(hipStreamSynchronize(st));
    }
    return DSP_OK;
}

long dsp_stop_train_used_features(const dsp_stop_trainer *t)
{
    if (const int rc = check_trainer(t)) return rc;
    return t->n ? t->shape.f_used : 0;
}

int dsp_stop_train_rows_host(dsp_stop_trainer *t, float *z, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (!z) return capi_fail(DSP_EINVAL, "z is NULL");
    if (t->n == 0) return capi_fail(DSP_EINVAL, "the trainer has no dataset (dsp_stop_train_set_device)");
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    if (t->shape.f_used) DSP_CAPI_HIP(hipMemcpyAsync(z, t->z.get(), (size_t)t->n * (size_t)t->shape.f_used * sizeof(float), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    return DSP_OK;
}

int dsp_stop_train_runs_device(dsp_stop_trainer *t, const dsp_stop_train_run *runs, long n_runs, const int *labels, dsp_stop_train_result *results,
                               double *d_history, double *d_prob, double *d_params, void *stream)
{
    if (const int rc = check_trainer(t)) return rc;
    if (n_runs < 0 || n_runs > dsp::kStopTrainMaxRuns) return capi_fail(DSP_EINVAL, "n_runs must be 0 .. 4096 (DSP_STOP_TRAIN_CAP_RUNS), got " + std::to_string(n_runs));
    if (n_runs && !runs) return capi_fail(DSP_EINVAL, "runs is NULL");
    if (n_runs && !results) return capi_fail(DSP_EINVAL, "results is NULL");
    if (n_runs && !d_history) return capi_fail(DSP_EINVAL, "d_history is NULL");
    if (n_runs && !d_params) return capi_fail(DSP_EINVAL, "d_params is NULL");
    if (!labels) return capi_fail(DSP_EINVAL, "labels is NULL");
    int max_epochs;
    if (const int rc = check_hyper(runs, n_runs, max_epochs)) return rc;
    if (t->n == 0) return capi_fail(DSP_EINVAL, "the trainer has no dataset (dsp_stop_train_set_device)");
    if (n_runs == 0) return DSP_OK;
    if (const int rc = check_labels(labels, t->n)) return rc;
    size_t total;
    if (const int rc = check_run_rows(runs, n_runs, t->n, total)) return rc;
    if (const int rc = dsp::check_device(t->device)) return rc;
    DSP_ON_DEVICE(t->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)t->n, P = (size_t)n_runs;
    const dsp::StopTrainShape &s = t->shape;
    // the runs' table, the labels and the row lists through the ring
    const size_t bytes = P * sizeof(dsp::StopTrainRun) + (n + total) * sizeof(int);
    dsp::SpanRing::Lease slot;
    if (const int rc = dsp::lease(t->spans, bytes, slot)) return rc;
    auto *h_run = static_cast<dsp::StopTrainRun *>(slot.h());
    int *h_labels = reinterpret_cast<int *>(h_run + P), *h_members = h_labels + n;
    std::memcpy(h_labels, labels, n * sizeof(int));
    size_t first = 0;
    for (size_t p = 0; p < P; ++p) {
        const dsp_stop_train_run &r = runs[p];
        dsp::StopTrainRun d{};
        d.train_first = (long)first;
        d.val_first = (long)(first + (size_t)r.n_train);
        d.n_train = (int)r.n_train;
        d.n_val = (int)r.n_val;
        d.seed = r.seed;
        d.lr = r.learning_rate;
        for (int l = 0; l < 3; ++l) { d.rate[l] = r.dropout[l]; d.keep_scale[l] = 1.0 / (1.0 - r.dropout[l]); }
        d.batch = r.batch_size; d.epochs = r.epochs; d.patience = r.patience; d.restore_best = r.restore_best;
        if (r.n_train) std::memcpy(h_members + first, r.train_rows, (size_t)r.n_train * sizeof(int));
        if (r.n_val) std::memcpy(h_members + first + (size_t)r.n_train, r.val_rows, (size_t)r.n_val * sizeof(int));
        first += (size_t)r.n_train + (size_t)r.n_val;
        h_run[p] = d;
    }
    const size_t state_bytes = (P * sizeof(dsp::StopTrainState) + 15) / 16 * 16, result_bytes = (P * sizeof(dsp_stop_train_result) + 15) / 16 * 16;
    if (t->table.reserve(state_bytes + result_bytes + P * sizeof(int)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the trainer's run table");
    if (t->slabs.reserve(P * dsp::stop_train_slab(s) * sizeof(double)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc of the runs' slabs");
    DSP_CAPI_HIP(slot.upload(bytes, st));
    const auto *d_run = static_cast<const dsp::StopTrainRun *>(slot.d());
    const int *d_labels = reinterpret_cast<const int *>(d_run + P), *d_members = d_labels + n;
    auto *d_state = reinterpret_cast<dsp::StopTrainState *>(t->table.get());
    auto *d_result = reinterpret_cast<dsp_stop_train_result *>(t->table.get() + state_bytes);
    int *d_stop = reinterpret_cast<int *>(t->table.get() + state_bytes + result_bytes);
    DSP_CAPI_HIP(dsp::launch_stop_train_init(s, d_run, n_runs, max_epochs, t->slabs, d_state, d_stop, d_history, st));
    std::vector<int> stopped(P);
    for (int epoch = 0; epoch < max_epochs; ++epoch) {
        DSP_CAPI_HIP(dsp::launch_stop_train_epoch(s, t->z, d_labels, d_members, d_run, n_runs, epoch, max_epochs, t->slabs, d_state, d_stop, d_history, st));
        if ((epoch + 1) % dsp::kStopTrainPoll == 0 && epoch + 1 < max_epochs) {
            DSP_CAPI_HIP(hipMemcpyAsync(stopped.data(), d_stop, P * sizeof(int), hipMemcpyDeviceToHost, st));
            DSP_CAPI_HIP(hipStreamSynchronize(st));
            if (std::all_of(stopped.begin(), stopped.end(), [](int v) { return v != 0; })) break;
        }
    }
    DSP_CAPI_HIP(dsp::launch_stop_train_finish(s, t->z, t->n, d_labels, d_members, d_run, n_runs, t->slabs, d_state, d_params, d_prob, d_result, st));
    DSP_CAPI_HIP(hipMemcpyAsync(results, d_result, P * sizeof(*results), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    return DSP_OK;
}

long dsp_stop_train_param_count(int n_coef, int max_frames, const int *units)
{
    if (const int rc = check_shape(n_coef, max_frames, units)) return rc;
    return dsp::stop_train_shape(n_coef, max_frames, units, 0).n_params;
}

double dsp_stop_train_uniform(unsigned long long seed, unsigned long long stream, unsigned long long counter)
{
    return dsp::stop_train_uniform(seed, stream, counter);
}

int dsp_stop_train_order(long n, unsigned long long seed, long epoch, int *order)
{
    if (!order) return capi_fail(DSP_EINVAL, "order is NULL");
    if (n < 1 || n > dsp::kStopTrainMaxRows) return capi_fail(DSP_EINVAL, "n must be 1 .. 65536, got " + std::to_string(n));
    if (epoch < 0) return capi_fail(DSP_EINVAL, "epoch must be >= 0");
    const uint64_t key = dsp::stop_train_draw(seed, 1, (uint64_t)epoch);
    for (long i = 0; i < n; ++i) order[i] = (int)dsp::stop_train_order_at((uint32_t)n, key, (uint32_t)i);
    return DSP_OK;
}

int dsp_stop_train_init(int n_coef, int max_frames, const int *units, unsigned long long seed, double *params)
{
    if (const int rc = check_shape(n_coef, max_frames, units)) return rc;
    if (!params) return capi_fail(DSP_EINVAL, "params is NULL");
    const dsp::StopTrainShape s = dsp::stop_train_shape(n_coef, max_frames, units, 0);
    long fan = s.n_in, k = 0;
    for (int l = 0; l < 4; ++l) {
        for (long e = 0; e < fan * units[l]; ++e, ++k) params[k] = dsp::stop_train_glorot(seed, (uint64_t)k, s.limit[l]);
        for (int e = 0; e < units[l]; ++e, ++k) params[k] = 0.0;
        fan = units[l];
    }
    return DSP_OK;
}

int dsp_stop_model_from_training(int n_coef, int max_frames, const int *units, const double *params, const float *mean, const float *scale,
                                 float *arrays, dsp_stop_model_params *model)
{
    if (const int rc = check_shape(n_coef, max_frames, units)) return rc;
    if (!params || !mean || !scale || !arrays || !model) return capi_fail(DSP_EINVAL, "params, mean, scale, arrays and model must not be NULL");
    const dsp::StopTrainShape s = dsp::stop_train_shape(n_coef, max_frames, units, 0);
    for (long k = 0; k < s.n_params; ++k)
        if (!std::isfinite(params[k])) return capi_fail(DSP_EINVAL, "params[" + std::to_string(k) + "] is not finite");
    model->n_coef = n_coef;
    model->max_frames = max_frames;
    std::memcpy(model->units, units, sizeof(model->units));
    std::memcpy(arrays, mean, (size_t)s.n_in * sizeof(float));
    std::memcpy(arrays + s.n_in, scale, (size_t)s.n_in * sizeof(float));
    model->scaler_mean = arrays;
    model->scaler_scale = arrays + s.n_in;
    float *w = arrays + 2 * s.n_in;
    long fan = s.n_in, k = 0;
    for (int l = 0; l < 4; ++l) {
        model->kernel[l] = w + k;
        for (long e = 0; e < fan * units[l]; ++e, ++k) w[k] = (float)params[k];
        model->bias[l] = w + k;
        for (int e = 0; e < units[l]; ++e, ++k) w[k] = (float)params[k];
        fan = units[l];
    }
    return DSP_OK;
}

}  // extern "C"
