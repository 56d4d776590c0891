// capi_consumers.cpp -- C ABI of the consumers of the MFCC matrix (stop-word net, speaker GMM) and of the
// linear resampler (include/dsp_amd.h).  Same rules as capi.cpp: models own
// device copies of their parameters, there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "consumer_kernels.hpp"
#include "mfcc_plan.hpp"

using dsp::capi_fail;
using dsp::scan_args;
using dsp::scan_plan;
using dsp::scan_upload;

struct dsp_stop_model : dsp::Handle {
    dsp::StopModelDev m{};
    dsp::DeviceBuf<void> d_blob;
    // workspace of dsp_classify_signal_batch_device / dsp_classify_signal
    dsp::DeviceBuf<float> d_mfcc, d_sig, d_prob;
    std::unique_ptr<dsp_mfcc_plan, dsp::DestroyWith<dsp_mfcc_plan_destroy>> plan;     // default plan of dsp_classify_signal (owned)
    std::mutex mu;
    dsp::SpanRing scan;      // dsp_stop_scan_device: the per-recording offsets on their way to the GPU
};

struct dsp_speaker_model : dsp::Handle {
    dsp::GmmDev target{}, ubm{};
    dsp::DeviceBuf<void> d_blob;
    dsp::SpanRing rows;      // dsp_speaker_llr_ragged_device, dsp_speaker_scan_device: the offsets on their way to the GPU (capi_util.hpp)
    // workspace of dsp_speaker_scan_device: the prefix sums of the per-row LLR (one stream at a time, include/dsp_amd.h)
    dsp::DeviceBuf<unsigned long long> d_scan;
    std::mutex mu;
};

// the model's device blob from parameters dsp_stop_model_create has accepted; the model's device is current
static int stop_model_init(dsp_stop_model *m, const dsp_stop_model_params *p)
{
    const size_t n_in = (size_t)p->n_coef * p->max_frames, u1 = p->units[0];
    // divisor with the reference's zero guard (audio_classifier_inference.c:44-45)
    std::vector<float> div(n_in);
    for (size_t i = 0; i < n_in; ++i) div[i] = p->scaler_scale[i] == 0.0f ? 1.0f : p->scaler_scale[i];
    // layer-1 contribution of the zero-padded frames: pad[T][j] = sum_{c, t >= T} W[c*max+t][j] * fl((0 - mean) / div)
    std::vector<double> pad((size_t)(p->max_frames + 1) * u1, 0.0);
    for (int t = p->max_frames - 1; t >= 0; --t)
        for (size_t j = 0; j < u1; ++j) {
            double s = pad[(size_t)(t + 1) * u1 + j];
            for (int c = 0; c < p->n_coef; ++c) {
                const size_t i = (size_t)c * p->max_frames + t;
                const float xs = (0.0f - p->scaler_mean[i]) / div[i];
                s += (double)p->kernel[0][i * u1 + j] * (double)xs;
            }
            pad[(size_t)t * u1 + j] = s;
        }
    // the fused epilogue's form of layer 1 (consumer_kernels.hpp): A = w / div per input, and per T the constant the live
    // inputs' B = -mean A add up to, on top of the padded frames' contribution
    const bool foldable = u1 <= (size_t)dsp::kStopFusedUnits;
    std::vector<float> fold_a;
    std::vector<double> pad_b;
    if (foldable) {
        fold_a.assign(n_in * dsp::kStopFusedUnits, 0.0f);
        pad_b.assign(pad.size(), 0.0);
        std::vector<double> live(u1, 0.0);                          // sum_{t' < t, c} B
        for (int t = 0; t <= p->max_frames; ++t) {
            for (size_t j = 0; j < u1; ++j) pad_b[(size_t)t * u1 + j] = pad[(size_t)t * u1 + j] + live[j];
            if (t == p->max_frames) break;
            for (int c = 0; c < p->n_coef; ++c) {
                const size_t i = (size_t)c * p->max_frames + t;
                for (size_t j = 0; j < u1; ++j) {
                    const double a = (double)p->kernel[0][i * u1 + j] / (double)div[i];
                    fold_a[i * dsp::kStopFusedUnits + j] = (float)a;
                    live[j] += -(double)p->scaler_mean[i] * (double)(float)a;      // B pairs with the ROUNDED A the kernel multiplies by
                }
            }
        }
    }
    // one device blob: doubles first (alignment), then floats
    size_t n_f = 2 * n_in + fold_a.size();
    size_t fan_in = n_in;
    for (int l = 0; l < 4; ++l) { n_f += fan_in * p->units[l] + p->units[l]; fan_in = p->units[l]; }
    const size_t bytes = (pad.size() + pad_b.size() + 1) * sizeof(double) + n_f * sizeof(float);
    if (m->d_blob.alloc(bytes) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc");
    std::vector<char> host(bytes);
    char *h = host.data();
    char *d = static_cast<char *>(m->d_blob.get());
    size_t off = 0;
    auto put = [&](const void *src, size_t n) { std::memcpy(h + off, src, n); const void *dev = d + off; off += n; return dev; };
    m->m.n_coef = p->n_coef;
    m->m.max_frames = p->max_frames;
    m->m.pad = static_cast<const double *>(put(pad.data(), pad.size() * sizeof(double)));
    m->m.pad_b = foldable ? static_cast<const double *>(put(pad_b.data(), pad_b.size() * sizeof(double))) : nullptr;
    if ((pad.size() + pad_b.size()) % 2) { static const double zero = 0.0; (void)put(&zero, sizeof(double)); }      // keep fold_a 16-byte aligned
    m->m.fold_a = foldable ? static_cast<const float *>(put(fold_a.data(), fold_a.size() * sizeof(float))) : nullptr;
    m->m.mean = static_cast<const float *>(put(p->scaler_mean, n_in * 4));
    m->m.div = static_cast<const float *>(put(div.data(), n_in * 4));
    fan_in = n_in;
    for (int l = 0; l < 4; ++l) {
        m->m.units[l] = p->units[l];
        m->m.kernel[l] = static_cast<const float *>(put(p->kernel[l], fan_in * p->units[l] * 4));
        m->m.bias[l] = static_cast<const float *>(put(p->bias[l], (size_t)p->units[l] * 4));
        fan_in = p->units[l];
    }
    if (hipMemcpy(m->d_blob, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return capi_fail(DSP_EHIP, "hipMemcpy");
    return DSP_OK;
}

extern "C" {

int dsp_stop_model_create(const dsp_stop_model_params *p, int device, dsp_stop_model **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (!p || p->n_coef <= 0 || p->max_frames <= 0 || !p->scaler_mean || !p->scaler_scale) return capi_fail(DSP_EINVAL, "bad stop-model parameters");
    for (int l = 0; l < 4; ++l)
        if (p->units[l] <= 0 || p->units[l] > dsp::kStopMaxUnits || !p->kernel[l] || !p->bias[l])
            return capi_fail(DSP_EINVAL, "stop-model layers must have 1..16 units and non-NULL parameters");
    if (p->units[3] != 1) return capi_fail(DSP_EINVAL, "the last layer must have one unit (sigmoid output)");
    if (const int rc = dsp::check_device(device)) return rc;
    return dsp::create_on_device(device, out, [&](dsp_stop_model &m) { return stop_model_init(&m, p); });
}

void dsp_stop_model_destroy(dsp_stop_model *m) { dsp::destroy(m); }

int dsp_stop_predict_device(dsp_stop_model *m, const float *d_mfcc, long n_clips, int frames_per_clip, float *d_prob, void *stream)
{
    if (!m || n_clips < 0 || frames_per_clip < 0 || (n_clips > 0 && (!d_prob || (frames_per_clip > 0 && !d_mfcc))))
        return capi_fail(DSP_EINVAL, "bad argument");
    DSP_CAPI_HIP(dsp::launch_stop_tail(m->m, d_mfcc, n_clips, frames_per_clip, d_prob, (hipStream_t)stream));
    return DSP_OK;
}

}  // extern "C"

// classify_signal in one kernel -- clip -> MFCC -> stop-word net, the MFCC matrix never written.  Returns 1 when the fused
// kernel was enqueued, 0 when this plan / model shape has no fused form (the caller runs the two-kernel path), < 0 on error.
// t = frames per clip (already capped at the model's max_frames).  offsets != nullptr: a ragged batch (clip c = samples [offsets[c],
// offsets[c + 1]) per channel; clip_stride and t unused)
static int stop_fused(dsp_mfcc_plan *p, const dsp::StopModelDev &m, const void *d_signal, int in_kind, long n_clips, long clip_stride, int t,
                      const long *offsets, float *d_prob, void *stream)
{
    if (offsets) { t = 1; clip_stride = 0; }
    if (const int fused = dsp::plan_accepts(p, dsp::PlanUse::FusedStop, in_kind); fused <= 0) return fused;
    if (m.n_coef != p->cfg.n_mfcc || m.units[0] > dsp::kStopFusedUnits || !m.fold_a || t <= 0 || std::getenv("DSP_AMD_STOP_TWO_KERNELS")) return 0;
    if (!dsp::input_aligned(d_signal, in_kind, n_clips > 1, clip_stride)) return 0;      // the two-kernel path reports it
    if (m.max_frames <= 0) return capi_fail(DSP_EINVAL, "stop model without frames");
    // ragged: frames past the model's max_frames are dropped (stop_detector.c:26-30): a clip's walk ends there
    const dsp::FusedClips c{.in = d_signal, .in_kind = in_kind, .n_clips = n_clips, .t = t, .clip_stride = clip_stride, .offsets = offsets,
                            .max_frames = m.max_frames, .stream = stream};
    const dsp::StopNetArgs stop{m, d_prob};
    const int rc = dsp::launch_fused_clips(p, c, nullptr, &stop);
    return rc < 0 ? rc : 1;
}

// classify_signal over a batch; in_kind 0 = float samples, 1 / 2 / 3 = int16 mono / stereo channel 0 / stereo average (what
// main_test.c:198-217 decodes in front of classify_signal, converted in the kernel's load)
static int classify_signal_batch(dsp_mfcc_plan *plan, dsp_stop_model *m, const void *d_signal, int in_kind, long n_clips, int samples_per_clip,
                                 long clip_stride, float *d_prob, void *stream)
{
    if (in_kind < 0) return in_kind;
    if (!plan || !m || n_clips < 0 || (n_clips > 0 && (!d_signal || !d_prob))) return capi_fail(DSP_EINVAL, "bad argument");
    const dsp_mfcc_config &cfg = plan->cfg;
    if (cfg.n_mfcc != m->m.n_coef) return capi_fail(DSP_EINVAL, "plan n_mfcc differs from the model's n_coef");
    // (the fused kernel is the default path: it must refuse what the two-kernel path refuses)
    if (n_clips > 1 && clip_stride < samples_per_clip) return capi_fail(DSP_EINVAL, "clip_stride < samples_per_clip");
    if (plan->device != m->device) return capi_fail(DSP_EINVAL, "plan and stop model live on different devices");
    if (n_clips == 0) return DSP_OK;
    const int t = dsp_mfcc_frames_for(&cfg, samples_per_clip, m->m.max_frames);          // stop_detector.c:18-21
    // one kernel from PCM to probability when the plan is the reference's shape
    if (const int fused = stop_fused(plan, m->m, d_signal, in_kind, n_clips, clip_stride, t, nullptr, d_prob, stream); fused != 0)
        return fused < 0 ? fused : DSP_OK;
    std::lock_guard<std::mutex> lock(m->mu);
    DSP_ON_DEVICE(m->device);
    DSP_CAPI_HIP(m->d_mfcc.reserve((size_t)n_clips * (t > 0 ? t : 1) * cfg.n_mfcc * sizeof(float)));
    if (t > 0) {
        const int rc = dsp::mfcc_clips(plan, d_signal, in_kind, n_clips, samples_per_clip, clip_stride, m->d_mfcc, m->m.max_frames, stream);
        if (rc < 0) return rc;
    }
    DSP_CAPI_HIP(dsp::launch_stop_tail(m->m, m->d_mfcc, n_clips, t, d_prob, (hipStream_t)stream));
    return DSP_OK;
}

extern "C" {

int dsp_classify_signal_batch_device(dsp_mfcc_plan *plan, dsp_stop_model *m, const float *d_signal, long n_clips,
                                     int samples_per_clip, long clip_stride, float *d_prob, void *stream)
{
    return classify_signal_batch(plan, m, d_signal, 0, n_clips, samples_per_clip, clip_stride, d_prob, stream);
}

int dsp_classify_signal_batch_pcm16_device(dsp_mfcc_plan *plan, dsp_stop_model *m, const int16_t *d_pcm, long n_clips, int samples_per_clip,
                                           long clip_stride, int channels, int stereo_mode, float *d_prob, void *stream)
{
    return classify_signal_batch(plan, m, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, samples_per_clip, clip_stride, d_prob, stream);
}

// Ragged batches (main_test.c:254-331 loops over files of different lengths): one launch of the fused kernel, every clip with the
// frames its own length gives (capped at the model's max_frames).  The fused kernel only: plans outside its shape are refused.
static int classify_signal_batch_ragged(dsp_mfcc_plan *plan, dsp_stop_model *m, const void *d_signal, int in_kind, long n_clips, const long *offsets,
                                        float *d_prob, void *stream)
{
    if (in_kind < 0) return in_kind;
    if (!plan || !m || n_clips < 0 || !offsets || (n_clips > 0 && (!d_signal || !d_prob))) return capi_fail(DSP_EINVAL, "bad argument");
    if (plan->cfg.n_mfcc != m->m.n_coef) return capi_fail(DSP_EINVAL, "plan n_mfcc differs from the model's n_coef");
    if (plan->device != m->device) return capi_fail(DSP_EINVAL, "plan and stop model live on different devices");
    if (n_clips == 0) return DSP_OK;
    const int fused = stop_fused(plan, m->m, d_signal, in_kind, n_clips, 0, 1, offsets, d_prob, stream);
    if (fused == 0) return capi_fail(DSP_EINVAL, "ragged batches run on the fused clip -> probability kernel: the reference's MFCC shape (dsp_mfcc_default_config), "
                                                 "a model with at most 4 first-layer units, an 8-byte aligned buffer (4 for mono int16)");
    return fused < 0 ? fused : DSP_OK;
}

int dsp_classify_signal_batch_ragged_device(dsp_mfcc_plan *plan, dsp_stop_model *m, const float *d_signal, long n_clips, const long *offsets,
                                            float *d_prob, void *stream)
{
    return classify_signal_batch_ragged(plan, m, d_signal, 0, n_clips, offsets, d_prob, stream);
}

int dsp_classify_signal_batch_ragged_pcm16_device(dsp_mfcc_plan *plan, dsp_stop_model *m, const int16_t *d_pcm, long n_clips, const long *offsets,
                                                  int channels, int stereo_mode, float *d_prob, void *stream)
{
    return classify_signal_batch_ragged(plan, m, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, d_prob, stream);
}

float dsp_classify_signal(dsp_stop_model *m, const float *signal, int num_samples)
{
    if (!m || !signal || num_samples < 0) { capi_fail(DSP_EINVAL, "bad argument"); return 0.0f; }
    auto bail = [](const char *what) { std::fprintf(stderr, "libdsp_amd: classify_signal: %s: %s\n", what, dsp_last_error()); return 0.0f; };
    {
        std::lock_guard<std::mutex> lock(m->mu);
        dsp::DeviceScope dsp_device_scope_(m->device);
        if (dsp_device_scope_.err != hipSuccess) { capi_fail(DSP_EHIP, "hipSetDevice"); return bail("device"); }
        if (!m->plan) {
            dsp_mfcc_config cfg;
            dsp_mfcc_default_config(&cfg);
            cfg.n_mfcc = m->m.n_coef;
            dsp_mfcc_plan *plan = nullptr;
            if (dsp_mfcc_plan_create(&cfg, m->device, &plan) < 0) return bail("plan");
            m->plan.reset(plan);
        }
        if (m->d_sig.reserve(((size_t)num_samples + 2) * sizeof(float)) != hipSuccess || m->d_prob.reserve(sizeof(float)) != hipSuccess) {
            capi_fail(DSP_ENOMEM, "hipMalloc");
            return bail("workspace");
        }
        if (num_samples > 0 && hipMemcpy(m->d_sig, signal, (size_t)num_samples * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            capi_fail(DSP_EHIP, "hipMemcpy");
            return bail("copy in");
        }
    }
    if (dsp_classify_signal_batch_device(m->plan.get(), m, m->d_sig, 1, num_samples, num_samples, m->d_prob, nullptr) < 0) return bail("run");
    float p = 0.0f;
    if (hipMemcpy(&p, m->d_prob, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { capi_fail(DSP_EHIP, "hipMemcpy"); return bail("copy out"); }
    return p;
}

int dsp_speaker_model_create(const dsp_gmm_params *target, const dsp_gmm_params *ubm, int device, dsp_speaker_model **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    for (const dsp_gmm_params *g : {target, ubm})
        if (!g || g->k <= 0 || g->k > 64 || g->d <= 0 || g->d > 16 || !g->means || !g->inv_covs || !g->log_consts)
            return capi_fail(DSP_EINVAL, "bad GMM parameters (k <= 64, d <= 16)");
    if (target->k != ubm->k || target->d != ubm->d) return capi_fail(DSP_EINVAL, "target and UBM must have the same shape");
    if (const int rc = dsp::check_device(device)) return rc;
    return dsp::create_on_device(device, out, [&](dsp_speaker_model &m) -> int {
        const size_t kd = (size_t)target->k * target->d, k = target->k;
        // layout: int32 inv_covs (t, u), int16 log_consts (t, u), int8 means (t, u)
        const size_t bytes = 2 * kd * 4 + 2 * k * 2 + 2 * kd;
        std::vector<char> host(bytes);
        if (m.d_blob.alloc(bytes) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc");
        char *d = static_cast<char *>(m.d_blob.get());
        size_t off = 0;
        auto put = [&](const void *src, size_t n) { std::memcpy(host.data() + off, src, n); const void *dev = d + off; off += n; return dev; };
        m.target.k = m.ubm.k = target->k;
        m.target.d = m.ubm.d = target->d;
        m.target.inv_covs = static_cast<const int32_t *>(put(target->inv_covs, kd * 4));
        m.ubm.inv_covs = static_cast<const int32_t *>(put(ubm->inv_covs, kd * 4));
        m.target.log_consts = static_cast<const int16_t *>(put(target->log_consts, k * 2));
        m.ubm.log_consts = static_cast<const int16_t *>(put(ubm->log_consts, k * 2));
        m.target.means = static_cast<const int8_t *>(put(target->means, kd));
        m.ubm.means = static_cast<const int8_t *>(put(ubm->means, kd));
        if (hipMemcpy(m.d_blob, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return capi_fail(DSP_EHIP, "hipMemcpy");
        return DSP_OK;
    });
}

void dsp_speaker_model_destroy(dsp_speaker_model *m) { dsp::destroy(m); }

int dsp_speaker_llr_device(dsp_speaker_model *m, const float *d_mfcc, long n_clips, int frames_per_clip, int64_t *d_llr_mean,
                           int *d_labels, int64_t *d_ll_target, int64_t *d_ll_ubm, void *stream)
{
    if (!m || n_clips < 0 || frames_per_clip <= 0 || (n_clips > 0 && (!d_mfcc || !d_llr_mean))) return capi_fail(DSP_EINVAL, "bad argument");
    const long long threshold = (long long)(-0.7 * (1 << 8));                              // speaker_gmm.c:124-125
    DSP_CAPI_HIP(dsp::launch_speaker_llr(m->target, m->ubm, d_mfcc, n_clips, frames_per_clip, threshold,
                                         reinterpret_cast<long long *>(d_llr_mean), d_labels, reinterpret_cast<long long *>(d_ll_target),
                                         reinterpret_cast<long long *>(d_ll_ubm), (hipStream_t)stream));
    return DSP_OK;
}

int dsp_speaker_llr_ragged_device(dsp_speaker_model *m, const float *d_mfcc, long n_clips, const long *frame_offsets, int64_t *d_llr_mean,
                                  int *d_labels, int64_t *d_ll_target, int64_t *d_ll_ubm, void *stream)
{
    if (!m || n_clips < 0 || (n_clips > 0 && (!frame_offsets || !d_mfcc || !d_llr_mean))) return capi_fail(DSP_EINVAL, "bad argument");
    if (n_clips == 0) return DSP_OK;
    if (frame_offsets[0] < 0) return capi_fail(DSP_EINVAL, "frame_offsets must be non-negative");
    for (long c = 0; c < n_clips; ++c)
        if (frame_offsets[c + 1] <= frame_offsets[c])
            return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + " of the ragged MFCC matrix has no frames (the LLR is a mean over the clip's frames)");
    DSP_ON_DEVICE(m->device);
    const size_t bytes = (size_t)(n_clips + 1) * sizeof(long);
    dsp::SpanRing::Lease slot;
    DSP_CAPI_HIP(m->rows.acquire(bytes, slot));
    std::memcpy(slot.h(), frame_offsets, bytes);
    DSP_CAPI_HIP(slot.upload(bytes, (hipStream_t)stream));
    const long long threshold = (long long)(-0.7 * (1 << 8));                              // speaker_gmm.c:124-125
    DSP_CAPI_HIP(dsp::launch_speaker_llr_ragged(m->target, m->ubm, d_mfcc, n_clips, static_cast<const long *>(slot.d()), threshold,
                                                reinterpret_cast<long long *>(d_llr_mean), d_labels, reinterpret_cast<long long *>(d_ll_target),
                                                reinterpret_cast<long long *>(d_ll_ubm), (hipStream_t)stream));
    return DSP_OK;
}

int dsp_upsample_linear_device(const float *d_in, long n_clips, int old_size, long in_stride, float *d_out, int new_size,
                               long out_stride, void *stream)
{
    if (n_clips < 0 || old_size < 1 || new_size < 2 || (n_clips > 0 && (!d_in || !d_out)) || (n_clips > 1 && (in_stride < old_size || out_stride < new_size)))
        return capi_fail(DSP_EINVAL, "bad argument (old_size >= 1, new_size >= 2)");
    for (long c0 = 0; c0 < n_clips; c0 += 65535) {
        const long cnt = n_clips - c0 < 65535 ? n_clips - c0 : 65535;
        DSP_CAPI_HIP(dsp::launch_upsample_linear(d_in + c0 * in_stride, cnt, old_size, in_stride, d_out + c0 * out_stride, new_size, out_stride,
                                                 (hipStream_t)stream));
    }
    return DSP_OK;
}

int dsp_upsample_linear_host(const float *in, int old_size, float *out, int new_size)
{
    if (!in || !out || old_size < 1 || new_size < 2) return capi_fail(DSP_EINVAL, "bad argument (old_size >= 1, new_size >= 2)");
    if (const int rc = dsp::check_device(0)) return rc;
    dsp::DeviceBuf<float> d_in, d_out;
    DSP_CAPI_HIP(d_in.alloc((size_t)old_size * 4));
    if (d_out.alloc((size_t)new_size * 4) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc");
    hipError_t e = hipMemcpy(d_in, in, (size_t)old_size * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsp::launch_upsample_linear(d_in, 1, old_size, old_size, d_out, new_size, new_size, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)new_size * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return capi_fail(DSP_EHIP, hipGetErrorString(e));
    return DSP_OK;
}

int dsp_fft_real_forward_host(const float *in_time, long n_frames, int frame_length, long in_stride, int n_fft, float *out_freq)
{
    if (!in_time || !out_freq || n_frames < 0 || (n_frames > 1 && in_stride < frame_length)) return capi_fail(DSP_EINVAL, "bad argument");
    if (n_fft < 2 || (n_fft & (n_fft - 1)) || n_fft > 4096 || frame_length < 1 || frame_length > n_fft) return capi_fail(DSP_EINVAL, "n_fft: a power of two <= 4096, 1 <= frame_length <= n_fft");
    if (n_frames == 0) return DSP_OK;
    if (const int rc = dsp::check_device(0)) return rc;
    dsp::DeviceBuf<float> d_in, d_out;
    DSP_CAPI_HIP(d_in.alloc((size_t)n_frames * frame_length * 4));
    if (d_out.alloc((size_t)n_frames * n_fft * 8) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc");
    hipError_t e = hipMemcpy2D(d_in, (size_t)frame_length * 4, in_time, (size_t)(n_frames > 1 ? in_stride : frame_length) * 4, (size_t)frame_length * 4, (size_t)n_frames, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dsp::launch_fft_real_forward(d_in, n_frames, frame_length, frame_length, n_fft, d_out, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out_freq, d_out, (size_t)n_frames * n_fft * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return capi_fail(DSP_EHIP, hipGetErrorString(e));
    return DSP_OK;
}

/* 2fa/audio/word/c/mfcc.c:16 (non-static there; SURVEY 8b lists it as an optional same-layer symbol): FRAME_LENGTH = 400 samples in,
 * MFCC_N_FFT = 512 complex bins out.  Same contract: void; a failure leaves the reason in dsp_last_error() and zeros in out_freq. */
void fft_real_forward(const float *in_time, float *out_freq)
{
    if (out_freq && dsp_fft_real_forward_host(in_time, 1, 400, 400, 512, out_freq) < 0) {
        std::fprintf(stderr, "libdsp_amd: fft_real_forward: %s\n", dsp_last_error());
        for (int i = 0; i < 1024; ++i) out_freq[i] = 0.0f;
    }
}

}  // extern "C"

// ---- scanning long recordings: P(stop) and the speaker LLR per sliding window of MFCC rows -------------------------------------------
// In the reference's MFCC shape (per-frame log reference, complete frames, no prefilter) a row depends on its own samples only, so window
// w of a recording is rows [w hop, w hop + window_frames) of the recording's ragged MFCC matrix, and each row is computed once.

extern "C" {

long dsp_scan_window_offsets(const dsp_scan_config *cfg, const long *frame_offsets, long n_recordings, long *window_offsets)
{
    return scan_plan(cfg, frame_offsets, n_recordings, window_offsets, nullptr, 1);
}

int dsp_stop_scan_device(dsp_stop_model *m, const float *d_mfcc, long n_recordings, const long *frame_offsets, const dsp_scan_config *cfg,
                         float *d_prob, void *stream)
{
    if (!m) return capi_fail(DSP_EINVAL, "model is NULL");
    long rc = scan_args(cfg, n_recordings);
    if (rc < 0 || n_recordings == 0) return (int)rc;
    if (!frame_offsets || !d_prob) return capi_fail(DSP_EINVAL, "frame_offsets and d_prob must not be NULL");
    const int tw = dsp::stop_scan_tile(m->m, cfg->window_frames, cfg->hop_frames);
    if (tw == 0) return capi_fail(DSP_EINVAL, "the stop model's window (min(window_frames, max_frames) rows of n_coef) does not fit the scan kernel's LDS");
    std::vector<long> wo((size_t)n_recordings + 1), to((size_t)n_recordings + 1);
    if ((rc = scan_plan(cfg, frame_offsets, n_recordings, wo.data(), to.data(), tw)) < 0) return (int)rc;
    const long rows = frame_offsets[n_recordings] - frame_offsets[0];
    if (rows > 0 && !d_mfcc) return capi_fail(DSP_EINVAL, "d_mfcc is NULL");
    DSP_ON_DEVICE(m->device);
    dsp::SpanRing::Lease slot;
    DSP_CAPI_HIP(scan_upload(m->scan, frame_offsets, n_recordings, wo.data(), to.data(), slot, stream));
    const long *d = static_cast<const long *>(slot.d());
    DSP_CAPI_HIP(dsp::launch_stop_scan(m->m, rows > 0 ? d_mfcc + frame_offsets[0] * m->m.n_coef : d_mfcc, n_recordings, d, d + (n_recordings + 1),
                                       d + 2 * (n_recordings + 1), to[(size_t)n_recordings], cfg->window_frames, cfg->hop_frames, tw, d_prob,
                                       (hipStream_t)stream));
    return DSP_OK;
}

int dsp_speaker_scan_device(dsp_speaker_model *m, const float *d_mfcc, long n_recordings, const long *frame_offsets, const dsp_scan_config *cfg,
                            int64_t *d_llr_mean, int *d_labels, void *stream)
{
    if (!m) return capi_fail(DSP_EINVAL, "model is NULL");
    long rc = scan_args(cfg, n_recordings);
    if (rc < 0 || n_recordings == 0) return (int)rc;
    if (!frame_offsets || !d_mfcc || !d_llr_mean) return capi_fail(DSP_EINVAL, "frame_offsets, d_mfcc and d_llr_mean must not be NULL");
    std::vector<long> wo((size_t)n_recordings + 1);
    if ((rc = scan_plan(cfg, frame_offsets, n_recordings, wo.data(), nullptr, 1)) < 0) return (int)rc;
    if ((rc = dsp::refuse_rowless(frame_offsets, n_recordings, " has no MFCC rows (the LLR is a mean over a window's rows)")) < 0) return (int)rc;
    const long rows = frame_offsets[n_recordings] - frame_offsets[0];
    std::lock_guard<std::mutex> lock(m->mu);
    DSP_ON_DEVICE(m->device);
    const size_t need = (size_t)(rows + (rows + dsp::kLlrScanChunk - 1) / dsp::kLlrScanChunk) * sizeof(unsigned long long);
    if (m->d_scan.reserve(need) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (speaker scan workspace)");
    dsp::SpanRing::Lease slot;
    DSP_CAPI_HIP(scan_upload(m->rows, frame_offsets, n_recordings, wo.data(), nullptr, slot, stream));
    const long *d = static_cast<const long *>(slot.d());
    const long long threshold = (long long)(-0.7 * (1 << 8));                              // speaker_gmm.c:124-125
    DSP_CAPI_HIP(dsp::launch_speaker_scan(m->target, m->ubm, d_mfcc + frame_offsets[0] * m->target.d, rows, n_recordings, d, d + (n_recordings + 1),
                                          wo[(size_t)n_recordings], cfg->window_frames, cfg->hop_frames, threshold, m->d_scan,
                                          reinterpret_cast<long long *>(d_llr_mean), d_labels, (hipStream_t)stream));
    return DSP_OK;
}

}  // extern "C"

// mfcc_plan.hpp: the front end and the models of a scanner / a stream session
int dsp::scan_front_check(const dsp_mfcc_plan *plan, int in_kind, const dsp_stop_model *stop, const dsp_speaker_model *speaker, const dsp_scan_config *cfg)
{
    const dsp_mfcc_config &pcfg = plan->cfg;
    if (const int rc = dsp::plan_accepts(plan, dsp::PlanUse::Scan, in_kind)) return rc;
    const int device = plan->device;
    if (stop && (pcfg.n_mfcc != stop->m.n_coef || stop->device != device))
        return capi_fail(DSP_EINVAL, "the stop model needs n_coef = the plan's n_mfcc, on the plan's device");
    if (speaker && (pcfg.n_mfcc != speaker->target.d || speaker->device != device))
        return capi_fail(DSP_EINVAL, "the speaker model needs d = the plan's n_mfcc, on the plan's device");
    if (stop && dsp::stop_scan_tile(stop->m, cfg->window_frames, cfg->hop_frames) == 0)
        return capi_fail(DSP_EINVAL, "the stop model's window (min(window_frames, max_frames) rows of n_coef) does not fit the scan kernel's LDS");
    return DSP_OK;
}

// every row of every recording of a scanner (mfcc_plan.hpp)
long dsp::ScannerCore::mfcc(const void *d_signal, int in_kind, long n, const long *offsets, const char *rowless_tail, void *stream)
{
    fo.resize((size_t)n + 1);
    const long rows = dsp_mfcc_ragged_frame_offsets(&plan->cfg, offsets, n, INT_MAX, fo.data());     // no cap: every row of every recording
    if (rows < 0) return rows;
    if (const int rc = rowless_tail ? dsp::refuse_rowless(fo.data(), n, rowless_tail) : DSP_OK) return rc;
    if (rows == 0) return 0;
    if (!d_signal) return capi_fail(DSP_EINVAL, "d_signal is NULL");
    DSP_ON_DEVICE(plan->device);
    if (d_mfcc.reserve((size_t)rows * plan->cfg.n_mfcc * sizeof(float)) != hipSuccess) return capi_fail(DSP_ENOMEM, "hipMalloc (scanner MFCC workspace)");
    const int rc = mfcc_clips_ragged(plan, d_signal, in_kind, n, offsets, INT_MAX, d_mfcc, stream);
    return rc < 0 ? rc : rows;
}

// A scanner: PCM -> ragged MFCC matrix in its own workspace -> the models' window scans, all on the caller's stream.
struct dsp_scanner : dsp::Handle {      // device: the plan's
    dsp::ScannerCore core;
    dsp_stop_model *stop = nullptr;
    dsp_speaker_model *spk = nullptr;
};

// in_kind 0 float samples, 1 / 2 / 3 int16, < 0 an error of dsp::pcm16_kind
static int scanner_run(dsp_scanner *s, const void *d_signal, int in_kind, long n, const long *offsets, float *d_prob, int64_t *d_llr_mean, int *d_labels,
                       void *stream)
{
    if (in_kind < 0) return in_kind;
    if (!s || n < 0) return capi_fail(DSP_EINVAL, "bad argument (scanner, n_recordings >= 0)");
    if (n == 0) return DSP_OK;
    if (!offsets) return capi_fail(DSP_EINVAL, "offsets is NULL");
    if (s->stop && !d_prob) return capi_fail(DSP_EINVAL, "the scanner has a stop model: d_prob must not be NULL");
    if (s->spk && !d_llr_mean) return capi_fail(DSP_EINVAL, "the scanner has a speaker model: d_llr_mean must not be NULL");
    std::lock_guard<std::mutex> lock(s->core.mu);
    const long rows = s->core.mfcc(d_signal, in_kind, n, offsets,
                                   s->spk ? " is shorter than one frame: the speaker LLR is a mean over a window's rows" : nullptr, stream);
    if (rows < 0) return (int)rows;
    if (s->stop) {
        const int rc = dsp_stop_scan_device(s->stop, s->core.d_mfcc, n, s->core.fo.data(), &s->core.cfg, d_prob, stream);
        if (rc < 0) return rc;
    }
    if (s->spk) {
        const int rc = dsp_speaker_scan_device(s->spk, s->core.d_mfcc, n, s->core.fo.data(), &s->core.cfg, d_llr_mean, d_labels, stream);
        if (rc < 0) return rc;
    }
    return DSP_OK;
}

extern "C" {

int dsp_scanner_create(dsp_mfcc_plan *plan, dsp_stop_model *stop, dsp_speaker_model *speaker, const dsp_scan_config *cfg, dsp_scanner **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (!plan) return capi_fail(DSP_EINVAL, "plan is NULL");
    if (!stop && !speaker) return capi_fail(DSP_EINVAL, "a scanner needs a stop model, a speaker model or both");
    if (const int rc = scan_args(cfg, 0)) return rc;
    if (const int rc = dsp::scan_front_check(plan, 0, stop, speaker, cfg)) return rc;
    return dsp::create_on_host(plan->device, out, [&](dsp_scanner &s) {
        s.core.plan = plan;
        s.core.cfg = *cfg;
        s.stop = stop;
        s.spk = speaker;
        return DSP_OK;
    });
}

void dsp_scanner_destroy(dsp_scanner *s) { dsp::destroy(s); }

int dsp_scanner_run_device(dsp_scanner *s, const float *d_signal, long n_recordings, const long *offsets, float *d_prob, int64_t *d_llr_mean,
                           int *d_labels, void *stream)
{
    return scanner_run(s, d_signal, 0, n_recordings, offsets, d_prob, d_llr_mean, d_labels, stream);
}

int dsp_scanner_run_pcm16_device(dsp_scanner *s, const int16_t *d_pcm, long n_recordings, const long *offsets, int channels, int stereo_mode,
                                 float *d_prob, int64_t *d_llr_mean, int *d_labels, void *stream)
{
    return scanner_run(s, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_recordings, offsets, d_prob, d_llr_mean, d_labels, stream);
}

}  // extern "C"
