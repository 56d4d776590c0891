// capi.cpp -- the C ABI of libdsp_amd.so (include/dsp_amd.h): the MFCC plans, the SVM and the fused paths.  The donut classifiers
// are capi_classify_f32.cpp and capi_classify_f64.cpp.
//
// Host side of the drop-in boundary: owns plans (device tables + staging
// buffers), validates arguments the way the reference does, and enqueues the
// gfx950 kernels.  No CPU fallback exists: without a HIP device every compute
// entry point fails and says why through dsp_last_error().
#include "diag_guard.hpp"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dsp_amd.h"
#include "capi_util.hpp"
#include "classify_kernels.hpp"
#include "mfcc_kernels.hpp"
#include "svm_kernels.hpp"
#include "tables.hpp"

#ifdef DSP_PF_STAMPS
namespace dsp { hipError_t read_pf_stamps(unsigned long long *host, int count); }      // mfcc_kernels.hip, diagnostic builds
#endif
#ifdef DSP_RC_STAMPS
namespace dsp { hipError_t read_rc_stamps(unsigned long long *host, int count); hipError_t read_bd_stamps(unsigned long long *host, int count); }      // classify_kernels.hip, diagnostic builds
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

}  // namespace

// error sink shared with the other translation units of the C ABI (capi_util.hpp)
namespace dsp { int capi_fail(int code, const std::string &msg) { return fail(code, msg); } }

namespace {

#define DSP_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(DSP_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));         \
    } while (0)

bool valid_cfg(const dsp_mfcc_config &c, std::string &why)
{
    if (c.sample_rate <= 0) { why = "sample_rate must be positive"; return false; }
    if (c.hop_length <= 0) { why = "hop_length must be positive"; return false; }
    if (c.frame_length < 2) { why = "frame_length must be at least 2"; return false; }
    if (c.n_mels < 1 || c.n_mfcc < 1) { why = "n_mels and n_mfcc must be positive"; return false; }
    if (c.frame_length & 1) { why = "frame_length must be even (8-byte aligned frame loads)"; return false; }
    if (c.hop_length & 1) { why = "hop_length must be even (8-byte aligned frame loads)"; return false; }
    if (!(c.fmax > c.fmin) || c.fmin < 0) { why = "need 0 <= fmin < fmax"; return false; }
    if (!(c.amin > 0)) { why = "amin must be positive"; return false; }
    if (c.log_mode != DSP_LOG_PER_FRAME_MAX && c.log_mode != DSP_LOG_GLOBAL_REF1 && c.log_mode != DSP_LOG_LOG10_FLOOR) { why = "unknown log_mode"; return false; }
    if (c.mel_norm != DSP_MELNORM_NONE && c.mel_norm != DSP_MELNORM_SLANEY && c.mel_norm != DSP_MELNORM_LIBROSA && c.mel_norm != DSP_MELNORM_AUBIO_SLANEY) { why = "unknown mel_norm"; return false; }
    if (c.spectrum != DSP_SPECTRUM_POWER && c.spectrum != DSP_SPECTRUM_MAGNITUDE) { why = "unknown spectrum"; return false; }
    if (c.framing != DSP_FRAMING_COMPLETE && c.framing != DSP_FRAMING_STREAM) { why = "unknown framing"; return false; }
    // the aubio-semantics options of cepstrum/scrubjay_infer.c's front end live on the 2048-point kernel
    if (c.n_fft != 2048 && (c.mel_norm == DSP_MELNORM_AUBIO_SLANEY || c.log_mode == DSP_LOG_LOG10_FLOOR || c.spectrum != DSP_SPECTRUM_POWER ||
                            c.framing != DSP_FRAMING_COMPLETE)) {
        why = "DSP_MELNORM_AUBIO_SLANEY, DSP_LOG_LOG10_FLOOR, DSP_SPECTRUM_MAGNITUDE and DSP_FRAMING_STREAM are implemented for n_fft = 2048";
        return false;
    }
    if (c.mel_norm == DSP_MELNORM_AUBIO_SLANEY && c.n_mels != 40) { why = "DSP_MELNORM_AUBIO_SLANEY is aubio's 40-filter bank: n_mels must be 40"; return false; }
    if (c.framing == DSP_FRAMING_STREAM && c.hop_length > c.frame_length) { why = "DSP_FRAMING_STREAM needs hop_length <= frame_length"; return false; }
    if (c.log_mode == DSP_LOG_GLOBAL_REF1 && c.n_fft == 1024) { why = "DSP_LOG_GLOBAL_REF1 is implemented for n_fft = 512 and 2048"; return false; }
    if (c.prefilter != DSP_PREFILTER_NONE && c.n_fft == 2048) { why = "the per-frame prefilter is implemented for n_fft = 512 and 1024"; return false; }
    if (c.frame_length > c.n_fft) { why = "frame_length must not exceed n_fft"; return false; }
    if (c.win_length < 0 || c.win_length > c.frame_length) { why = "win_length must be in [0, frame_length]"; return false; }
    if (c.prefilter != DSP_PREFILTER_NONE && c.prefilter != DSP_PREFILTER_BUTTER_1000_3000 &&
        c.prefilter != DSP_PREFILTER_BUTTER_3000_7500) { why = "unknown prefilter"; return false; }
    if (c.n_fft != 512 && c.n_fft != 1024 && c.n_fft != 2048) { why = "n_fft must be 512, 1024 or 2048"; return false; }
    return true;
}

}  // namespace

struct dsp_mfcc_plan {
    dsp_mfcc_config cfg;
    int device = 0;
    int n_cu = 0;
    int resident_blocks = 4; // 256-thread blocks one CU holds (occupancy query), tile epilogue kernel
    int resident_blocks_frame = 4;   // same, per-frame epilogue kernel
    int blocks_per_cu = 0;   // 0 = default (= resident_blocks)
    int chunk = 0;           // 0 = default
    dsp::LaneTables512 host;
    dsp::DeviceBuf<dsp::LaneTables512> d_tables;
    dsp::DeviceBuf<dsp::RowTables512> d_row_tables;
    dsp::DeviceBuf<dsp::GenTables1024> d_gen_tables;   // n_fft = 1024
    dsp::DeviceBuf<dsp::GenTables2048> d_tables2048;   // n_fft = 2048
    dsp::DeviceBuf<dsp::PairExtra512> d_pair;          // n_fft = 512: extra constants of the two-frames-per-wave kernel (DSP_KERNEL_PAIR)
    int resident_blocks_pair = 3;
    int resident_blocks_2048 = 2, resident_blocks_2048_pool = 2;
    int resident_blocks_gen = 3;
    int gen_slots = 0;                            // mel chunk slots per lane the 1024-point tables use (<= 3: wave kernel)
    int resident_blocks_gen_wave = 2;
    dsp::DeviceBuf<dsp::PrefilterScan> d_scan;    // prefilter fused into the 1024-point wave kernel (full frames): its tables
    int scan_steps[4] = {6, 6, 6, 6};             // host copy of PrefilterScan::c_steps (picks the kernel instantiation)
    int resident_blocks_gen_pre = 2;
    dsp::DeviceBuf<float> d_filtered;             // per-frame prefilter output (sub-batch)
    dsp::DeviceBuf<float> d_frame_max, d_clip_floor;   // DSP_LOG_GLOBAL_REF1 two-pass workspace
    int kernel = DSP_KERNEL_WAVE;
    bool aub = false;                             // n_fft = 2048 with aubio's semantics (magnitude spectrum, log10 floor or stream framing)
    int resident_blocks_row = 3;
    // staging for the host-pointer entry points
    dsp::DeviceBuf<float> d_in, d_out;
    // Guards the plan's workspaces (d_filtered, d_frame_max / d_clip_floor, d_in / d_out) while a call reserves them and
    // enqueues the kernels that use them.  The kernels themselves run after the lock is released: a plan whose path uses
    // a workspace (prefilter, DSP_LOG_GLOBAL_REF1 over clips, the *_host entry points) serves ONE stream at a time;
    // the workspace-free paths (frames / clips / pcm16 / fused, per-frame log mode) may be driven from several streams.
    std::recursive_mutex mu;
    dsp::SpanRing spans;      // ragged batches of the fused clip kernels: the clips' spans on their way to the GPU (capi_util.hpp)
};

extern "C" {

const char *dsp_last_error(void) { return g_err.c_str(); }
#ifndef DSP_AMD_SRC_HASH
#define DSP_AMD_SRC_HASH "unknown"
#endif
#ifdef DSP_AMD_EXPERIMENTS
#define DSP_AMD_EXPERIMENTS_TAG " +experiments"
#else
#define DSP_AMD_EXPERIMENTS_TAG ""
#endif
const char *dsp_version(void) { return "dsp_amd 0.3 (gfx950)" DSP_AMD_EXPERIMENTS_TAG " src:" DSP_AMD_SRC_HASH; }

int dsp_abi_sizeof(int which)
{
    switch (which) {
    case 0: return (int)sizeof(dsp_mfcc_config);
    case 1: return (int)sizeof(dsp_classify_trace);
    case 2: return (int)sizeof(dsp_classify_trace_f64);
    default: return -1;
    }
}

int dsp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void dsp_mfcc_default_config(dsp_mfcc_config *c)
{
    // 2fa/audio/word/c/mfcc_params.h:6-12, mfcc.c:172-173, export_mfcc_params.py:44-57
    c->sample_rate = 16000;
    c->n_fft = 512;
    c->frame_length = 400;
    c->hop_length = 160;
    c->n_mels = 40;
    c->n_mfcc = 13;
    c->window = DSP_WINDOW_HANN;
    c->mel_norm = DSP_MELNORM_NONE;
    c->log_mode = DSP_LOG_PER_FRAME_MAX;
    c->prefilter = DSP_PREFILTER_NONE;
    c->spectrum = DSP_SPECTRUM_POWER;
    c->framing = DSP_FRAMING_COMPLETE;
    c->win_length = 0;
    c->fmin = 0.0f;
    c->fmax = 8000.0f;
    c->amin = 1e-10f;
    c->top_db = 80.0f;
}

void dsp_mfcc_scrubjay_infer_config(dsp_mfcc_config *c, int sample_rate)
{
    // cepstrum/scrubjay_infer.c:9-13 (N_MFCC 20, WIN_SIZE 2048, HOP_SIZE 1024, N_FILTERS 40), :28-30 (new_aubio_pvoc, new_aubio_mfcc)
    dsp_mfcc_default_config(c);
    c->sample_rate = sample_rate;
    c->n_fft = 2048;
    c->frame_length = 2048;
    c->hop_length = 1024;
    c->n_mels = 40;
    c->n_mfcc = 20;
    c->window = DSP_WINDOW_HANN;                 // new_aubio_window("hanningz"): the periodic Hann
    c->mel_norm = DSP_MELNORM_AUBIO_SLANEY;
    c->log_mode = DSP_LOG_LOG10_FLOOR;
    c->spectrum = DSP_SPECTRUM_MAGNITUDE;
    c->framing = DSP_FRAMING_STREAM;
    c->fmin = 0.0f;
    c->fmax = 0.5f * (float)sample_rate;         // not used by the aubio bank
}

int dsp_mfcc_frames_for(const dsp_mfcc_config *cfg, int num_samples, int max_frames)
{
    if (!cfg || max_frames <= 0) return 0;
    if (cfg->framing == DSP_FRAMING_STREAM) {
        // cepstrum/scrubjay_infer.c:39-53: a frame per aubio_source_do that returned samples
        if (num_samples <= 0) return 0;
        const long t = ((long)num_samples + cfg->hop_length - 1) / cfg->hop_length;
        return (int)std::min<long>(t, max_frames);
    }
    // mfcc.c:117-119, 132-139
    if (num_samples < cfg->frame_length) return 0;
    const int t = 1 + (num_samples - cfg->frame_length) / cfg->hop_length;
    return std::min(t, max_frames);
}

int dsp_mfcc_tables(const dsp_mfcc_config *cfg, float *window, float *mel, float *dct)
{
    if (!cfg) return fail(DSP_EINVAL, "cfg is NULL");
    {   // (the sanitizer tier's sweep found this entry point building tables for configurations dsp_mfcc_plan_create refuses --
        // sample_rate 0, fmin > fmax, n_fft 333: NaN tables rather than an error)
        std::string why;
        if (!valid_cfg(*cfg, why)) return fail(DSP_EINVAL, why);
    }
    if (window) {
        auto w = dsp::make_frame_window(*cfg);
        std::memcpy(window, w.data(), w.size() * sizeof(float));
    }
    if (mel) {
        auto m = dsp::make_mel_filterbank(cfg->sample_rate, cfg->n_fft, cfg->n_mels, cfg->fmin, cfg->fmax, cfg->mel_norm);
        std::memcpy(mel, m.data(), m.size() * sizeof(float));
    }
    if (dct) {
        auto d = dsp::make_dct_ortho(cfg->n_mfcc, cfg->n_mels);
        std::memcpy(dct, d.data(), d.size() * sizeof(float));
    }
    return DSP_OK;
}

int dsp_prefilter_scan_check(int prefilter, int *steps4)
{
    if (prefilter != DSP_PREFILTER_BUTTER_1000_3000 && prefilter != DSP_PREFILTER_BUTTER_3000_7500) return fail(DSP_EINVAL, "prefilter must name one of the two literal band-passes");
    double b[9], a[9];
    dsp_butter_bandpass(prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 1000 : 3000, prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 3000 : 7500, b, a);
    dsp::PrefilterScan sc;
    std::string why;
    if (!dsp::build_prefilter_scan(b, a, sc, why)) return fail(DSP_EINVAL, why);
    if (steps4) for (int k = 0; k < 4; ++k) steps4[k] = sc.c_steps[k];
    return (sc.c_ok ? 1 : 0) | (sc.c_row_ok ? 2 : 0);
}

int dsp_mfcc_lane_tables(const dsp_mfcc_config *cfg, void *out, int size)
{
    if (!cfg) return fail(DSP_EINVAL, "cfg is NULL");
    if (!out) return (int)sizeof(dsp::LaneTables512);
    if (size != (int)sizeof(dsp::LaneTables512)) return fail(DSP_EINVAL, "size != sizeof(LaneTables512)");
    std::string why;
    auto *t = new dsp::LaneTables512;
    const bool ok = valid_cfg(*cfg, why) && dsp::build_lane_tables_512(*cfg, *t, why);
    if (ok) std::memcpy(out, t, sizeof(*t));
    delete t;
    return ok ? DSP_OK : fail(DSP_EINVAL, why);
}

int dsp_butter_bandpass(double lowcut, double highcut, double *b, double *a)
{
    // donut-classifier/classifier.c:342-360, 383-401: the 16 kHz literal tables
    static const double B1[9] = {0.01020948, 0., -0.04083792, 0., 0.06125688, 0., -0.04083792, 0., 0.01020948};
    static const double A1[9] = {1., -4.56803686, 9.95922498, -13.49912589, 12.43979269, -7.94997696, 3.43760562, -0.92305481, 0.1203896};
    static const double B2[9] = {0.1362017, 0., -0.5448068, 0., 0.8172102, 0., -0.5448068, 0., 0.1362017};
    static const double A2[9] = {1., 2.60935592, 2.32553038, 1.20262614, 1.11690211, 0.76154474, 0.10005124, -0.0129829, 0.02236815};
    const double *sb, *sa;
    if (lowcut == 1000 && highcut == 3000) { sb = B1; sa = A1; }
    else if (lowcut == 3000 && highcut == 7500) { sb = B2; sa = A2; }
    else { fail(DSP_EINVAL, "invalid bandpass range"); return 0; }   // classifier.c:402-407
    std::memcpy(b, sb, sizeof(B1));
    std::memcpy(a, sa, sizeof(A1));
    return 1;
}

int dsp_mfcc_plan_create(const dsp_mfcc_config *cfg, int device, dsp_mfcc_plan **out)
{
    if (!cfg || !out) return fail(DSP_EINVAL, "cfg/out is NULL");
    *out = nullptr;
    std::string why;
    if (!valid_cfg(*cfg, why)) return fail(DSP_EINVAL, why);
    auto host_side = std::make_unique<dsp_mfcc_plan>();
    host_side->cfg = *cfg;
    std::unique_ptr<dsp::GenTables1024> gen;
    std::unique_ptr<dsp::GenTables2048> g2k;
    if (cfg->n_fft == 2048) {
        g2k = std::make_unique<dsp::GenTables2048>();
        if (!dsp::build_gen_tables_2048(*cfg, *g2k, why)) return fail(DSP_EINVAL, why);
    } else if (cfg->n_fft == 1024) {
        gen = std::make_unique<dsp::GenTables1024>();
        if (!dsp::build_gen_tables_1024(*cfg, *gen, why)) return fail(DSP_EINVAL, why);
    } else if (!dsp::build_lane_tables_512(*cfg, host_side->host, why)) return fail(DSP_EINVAL, why);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(DSP_ENODEV, "no HIP device: libdsp_amd has no CPU fallback");
    if (device < 0 || device >= n) return fail(DSP_EINVAL, "device index out of range");
    dsp::DeviceScope dsp_device_scope_(device);      // the caller's current device is put back on return
    // the plan gets device buffers from here on: its owner is declared after the scope, so that every exit below lets them go
    // while the plan's device is current
    std::unique_ptr<dsp_mfcc_plan> p = std::move(host_side);
    p->device = device;
    hipError_t e = dsp_device_scope_.err;
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) e = dsp::upload(p->d_tables, p->host);
    if (e == hipSuccess && gen) e = dsp::upload(p->d_gen_tables, *gen);
    if (e == hipSuccess && g2k) e = dsp::upload(p->d_tables2048, *g2k);
    if (gen) p->gen_slots = gen->n_chunk_slots;
    if (e == hipSuccess && cfg->n_fft == 1024 && cfg->prefilter != DSP_PREFILTER_NONE && cfg->frame_length == 1024 && p->gen_slots <= 3) {
        // BASELINE config 3 in ONE pass: the per-frame Butterworth as a scan inside the MFCC kernel (tables.hpp PrefilterScan)
        double b[9], a[9];
        dsp_butter_bandpass(cfg->prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 1000 : 3000,
                            cfg->prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 3000 : 7500, b, a);
        dsp::PrefilterScan sc;
        if (!dsp::build_prefilter_scan(b, a, sc, why)) return fail(DSP_EINVAL, why);
        if (sc.c_ok && (!DSP_PRE_ROWSCAN || sc.c_row_ok)) {      // the kernel runs the cascade form (its scan in row form); coefficients without it (none of the two literal sets) take the two-pass path
            e = dsp::upload(p->d_scan, sc);
            for (int k = 0; k < 4; ++k) p->scan_steps[k] = sc.c_steps[k];
        }
    }
#ifdef DSP_AMD_EXPERIMENTS
    // measured dead ends kept buildable (python -m dsp_amd.build with DSP_AMD_EXPERIMENTS=1): the row-per-frame kernel and
    // the two-frames-per-wave kernel; the default library does not carry them
    if (e == hipSuccess && cfg->n_fft == 512) {
        auto rt = std::make_unique<dsp::RowTables512>();
        dsp::build_row_tables_512(*cfg, *rt);
        e = dsp::upload(p->d_row_tables, *rt);
    }
    if (e == hipSuccess && cfg->n_fft == 512) {
        dsp::PairExtra512 px;
        dsp::build_pair_extra_512(px);
        e = dsp::upload(p->d_pair, px);
    }
#endif
    if (e != hipSuccess) return fail(DSP_EHIP, std::string("plan_create: ") + hipGetErrorString(e));
    p->n_cu = prop.multiProcessorCount;
    p->aub = cfg->n_fft == 2048 && (cfg->spectrum != DSP_SPECTRUM_POWER || cfg->log_mode == DSP_LOG_LOG10_FLOOR || cfg->framing == DSP_FRAMING_STREAM);
    if (cfg->n_fft == 2048) {
        p->resident_blocks_2048 = dsp::mfcc2048_blocks_per_cu(cfg->n_mels, false, p->aub);
        p->resident_blocks_2048_pool = dsp::mfcc2048_blocks_per_cu(cfg->n_mels, true, p->aub);
    } else if (cfg->n_fft == 512) {
        p->resident_blocks_frame = dsp::mfcc512_blocks_per_cu(p->host.dct_split, p->host.dct_len, p->host.mel_gather,
                                                              cfg->frame_length == 512, false);
        p->resident_blocks = dsp::mfcc512_blocks_per_cu(p->host.dct_split, p->host.dct_len, p->host.mel_gather,
                                                        cfg->frame_length == 512, true);
#ifdef DSP_AMD_EXPERIMENTS
        p->resident_blocks_row = dsp::mfcc512_row_blocks_per_cu(p->host.dct_split, p->host.dct_len, p->host.mel_gather,
                                                                cfg->frame_length == 512);
        p->resident_blocks_pair = dsp::mfcc512_pair_blocks_per_cu();
#endif
    } else {
        p->resident_blocks_gen = dsp::mfcc1024_blocks_per_cu(cfg->frame_length == 1024);
        p->resident_blocks_gen_wave = dsp::mfcc1024_wave_blocks_per_cu(cfg->frame_length == 1024);
        if (p->d_scan) p->resident_blocks_gen_pre = dsp::mfcc1024_wave_blocks_per_cu(true, true);
    }
    if (const char *k = std::getenv("DSP_AMD_KERNEL")) {
        // an A/B switch, not a requirement: a value this build (or this plan's n_fft) has no kernel for is reported and ignored --
        // an environment left over from an experiments build must not make every plan_create fail
        if (dsp_mfcc_plan_set_kernel(p.get(), std::atoi(k)) != DSP_OK)
            std::fprintf(stderr, "libdsp_amd: DSP_AMD_KERNEL=%s ignored (%s); using the default kernel\n", k, dsp_last_error());
    }
    *out = p.release();
    return DSP_OK;
}

void dsp_mfcc_plan_destroy(dsp_mfcc_plan *p)
{
    if (!p) return;
    dsp::DeviceScope dsp_device_scope_(p->device);
    p->spans.release();
    delete p;
}

int dsp_mfcc_plan_config(const dsp_mfcc_plan *p, dsp_mfcc_config *cfg)
{
    if (!p || !cfg) return fail(DSP_EINVAL, "plan/cfg is NULL");
    *cfg = p->cfg;
    return DSP_OK;
}

int dsp_mfcc_plan_set_kernel(dsp_mfcc_plan *p, int kernel)
{
    if (!p || (kernel != DSP_KERNEL_WAVE && kernel != DSP_KERNEL_ROW && kernel != DSP_KERNEL_WAVE_FRAME && kernel != DSP_KERNEL_PAIR)) return fail(DSP_EINVAL, "bad kernel id");
#ifndef DSP_AMD_EXPERIMENTS
    // DSP_KERNEL_ROW on a 1024-point plan selects the general Stockham kernel (a product path: the fallback for filterbanks
    // the wave kernel's tables do not hold); the 512-point row / pair kernels are experiments outside the default build
    if (kernel == DSP_KERNEL_PAIR || (kernel == DSP_KERNEL_ROW && p->cfg.n_fft != 1024))
        return fail(DSP_EINVAL, "DSP_KERNEL_ROW / DSP_KERNEL_PAIR (512-point experiments) are not in this build: rebuild with DSP_AMD_EXPERIMENTS=1");
#endif
    p->kernel = kernel;
    return DSP_OK;
}

int dsp_mfcc_plan_set_launch(dsp_mfcc_plan *p, int blocks_per_cu, int frames_per_chunk)
{
    if (!p || blocks_per_cu < 0 || frames_per_chunk < 0) return fail(DSP_EINVAL, "bad launch knobs");
    p->blocks_per_cu = blocks_per_cu;
    p->chunk = frames_per_chunk;
    return DSP_OK;
}

}  // extern "C"

// A ragged batch for run(): clip c = samples [offsets[c], offsets[c + 1]) per channel -- or [offsets[c], offsets[c] + lengths[c]) when
// lengths is given (spans anywhere in the buffer, overlapping ones included) -- frame_offsets[c] its first output row (prefix sums of the
// clips' frame counts), n_spans the clips with at least one frame.
struct RaggedBatch {
    const long *offsets, *frame_offsets;
    long n_clips, n_spans;
    const long *lengths = nullptr;
};

// ragged: the spans (caller's order, clips of >= 1 frame, ClipSpan::frame0 = first output row) and behind them the chunk table of the
// kernels' RaggedCursor (built on the device for `chunk`), in the leased ring slot
static int ragged_mfcc_spans(dsp_mfcc_plan *p, const RaggedBatch &rg, long n_frames, int chunk, dsp::SpanRing::Lease &slot, hipStream_t st)
{
    const size_t span_bytes = (size_t)rg.n_spans * sizeof(dsp::ClipSpan);
    const long n_chunks = (n_frames + chunk - 1) / chunk;
    DSP_HIP(p->spans.acquire(span_bytes + (size_t)n_chunks * sizeof(int), slot));
    auto *h = static_cast<dsp::ClipSpan *>(slot.h());
    long j = 0;
    for (long c = 0; c < rg.n_clips; ++c) {
        const int frames = (int)(rg.frame_offsets[c + 1] - rg.frame_offsets[c]);
        const long n = rg.lengths ? rg.lengths[c] : rg.offsets[c + 1] - rg.offsets[c];
        if (frames > 0) h[j++] = dsp::ClipSpan{rg.offsets[c], (int)n, frames, c, rg.frame_offsets[c]};
    }
    DSP_HIP(slot.upload(span_bytes, st));
    DSP_HIP(dsp::launch_ragged_chunk_map(static_cast<const dsp::ClipSpan *>(slot.d()), rg.n_spans, chunk,
                                         reinterpret_cast<int *>(static_cast<char *>(slot.d()) + span_bytes), st));
    return DSP_OK;
}

// the launch fields every path takes from the plan (clip_mode: stream framing applies to clips; independent frames are whole frames)
static dsp::Mfcc512Args plan_args(const dsp_mfcc_plan *p, const void *d_in, int in_kind, bool clip_mode)
{
    dsp::Mfcc512Args a{};
    a.in = d_in;
    a.in_kind = in_kind;
    a.tables = p->d_tables;
    a.hop = p->cfg.hop_length;
    a.frame_len = p->cfg.frame_length;
    a.n_mels = p->cfg.n_mels;
    a.n_mfcc = p->cfg.n_mfcc;
    a.amin = p->cfg.amin;
    a.top_db = p->cfg.top_db;
    a.log_mode = p->cfg.log_mode;
    a.spectrum = p->cfg.spectrum;
    a.stream_framing = clip_mode && p->cfg.framing == DSP_FRAMING_STREAM;
    return a;
}

// persistent-style grid: exactly the 4-wave blocks the chip holds at once (per_cu per CU unless dsp_mfcc_plan_set_launch says otherwise;
// one extra block per CU would run as a second, mostly idle round: measured +14 %), never more blocks than `items` of work fill
static int grid(const dsp_mfcc_plan *p, int per_cu, long items)
{
    return (int)std::max(1L, std::min((long)p->n_cu * (p->blocks_per_cu > 0 ? p->blocks_per_cu : per_cu), (items + 3) / 4));
}

// DSP_LOG_GLOBAL_REF1 over clips (clip-global top_db): pass 1 writes each frame's maximum, a tiny kernel turns them into one floor per
// clip, pass 2 is the normal kernel clipping at that floor.  launch(args) enqueues the plan's MFCC kernel.
template <class Launch> static int two_pass_floor(dsp_mfcc_plan *p, dsp::Mfcc512Args &a, hipStream_t st, const Launch &launch)
{
    const long n_clips = a.spans ? a.n_clips : a.n_frames / a.frames_per_clip;
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_HIP(p->d_frame_max.reserve((size_t)a.n_frames * sizeof(float)));
    DSP_HIP(p->d_clip_floor.reserve((size_t)n_clips * sizeof(float)));
    a.frame_max = p->d_frame_max;
    DSP_HIP(launch(a));
    if (a.spans) DSP_HIP(dsp::launch_clip_floor_ragged(p->d_frame_max, a.spans, n_clips, a.top_db, p->d_clip_floor, st));
    else DSP_HIP(dsp::launch_clip_floor(p->d_frame_max, n_clips, a.frames_per_clip, a.top_db, p->d_clip_floor, st));
    a.frame_max = nullptr;
    a.clip_floor = p->d_clip_floor;
    DSP_HIP(launch(a));
    return DSP_OK;
}

// rg != nullptr: a ragged batch (frames_per_clip = 0, clip_stride unused): the clip-mode kernels with the RaggedCursor
static int run(dsp_mfcc_plan *p, const void *d_in, float *d_out, long n_frames, int frames_per_clip,
               long clip_stride, void *stream, int in_kind = 0, bool fused_prefilter = false, int samples_per_clip = 0,
               const RaggedBatch *rg = nullptr)
{
    if (n_frames == 0) return DSP_OK;
    DSP_ON_DEVICE(p->device);       // the caller's current device may be another GPU: tables and workspaces live on the plan's
    hipStream_t st = (hipStream_t)stream;
    const bool clip_mode = frames_per_clip > 0 || rg;
    const bool single_clip = frames_per_clip > 0 && n_frames == frames_per_clip;   // stride unused
    if ((reinterpret_cast<uintptr_t>(d_in) & (in_kind == 1 ? 3 : 7)) || (!single_clip && (clip_stride & 1)))
        return fail(DSP_EINVAL, "input must be 8-byte aligned (4 for mono int16) with an even clip stride");
    if (in_kind != 0 && !(p->aub && clip_mode) && (p->cfg.n_fft != 512 || p->kernel != DSP_KERNEL_WAVE || p->cfg.log_mode != DSP_LOG_PER_FRAME_MAX))
        return fail(DSP_EINVAL, "PCM16 ingestion runs on the 512-point wave-per-frame kernel (per-frame log mode) and on the 2048-point scrubjay_infer.c front end");
    dsp::Mfcc512Args a = plan_args(p, d_in, in_kind, clip_mode);
    a.out = d_out;
    a.n_frames = n_frames;
    a.clip_stride = clip_stride;
    a.frames_per_clip = frames_per_clip;
    a.samples_per_clip = samples_per_clip;
    const bool fft2048 = p->cfg.n_fft == 2048, gen = p->cfg.n_fft == 1024;
#ifdef DSP_AMD_EXPERIMENTS
    const bool row = !gen && p->kernel == DSP_KERNEL_ROW && p->cfg.n_fft == 512;
    // two frames per wavefront step (experiment): the reference shape on independent full frames only, else the default form
    const bool pair = !gen && p->kernel == DSP_KERNEL_PAIR && p->d_pair && in_kind == 0 && frames_per_clip == 0 && p->cfg.frame_length == 512 &&
                      p->cfg.log_mode == DSP_LOG_PER_FRAME_MAX && p->host.dct_split == 4 && p->host.dct_len == 10 && p->host.mel_gather == 3;
#else
    const bool row = false, pair = false;
#endif
    // 16-frame tile epilogue: per-frame log mode on the wave-per-frame kernel
    const bool tile = !gen && (p->kernel == DSP_KERNEL_WAVE || p->kernel == DSP_KERNEL_PAIR) && p->cfg.log_mode == DSP_LOG_PER_FRAME_MAX;
    // 1024-point: the register-resident wave kernel when the filterbank fits two chunk slots per lane (DSP_KERNEL_ROW selects
    // the general Stockham kernel for A/B)
    const bool gen_wave = gen && p->gen_slots <= 3 && p->kernel != DSP_KERNEL_ROW;
    int per_cu;
    if (fft2048) {
        if (a.stream_framing && samples_per_clip <= 0 && !rg) return fail(DSP_EINVAL, "internal: stream framing without the clip length");
        a.chunk = p->chunk > 0 ? p->chunk : 8;
        per_cu = p->resident_blocks_2048;
    } else {
        const int nf = gen ? (gen_wave ? 8 : 1) : (pair ? 16 : (row ? 4 : (tile ? 8 : 1)));
        a.chunk = p->chunk > 0 ? p->chunk : (pair ? 16 : 8);
        a.chunk = ((a.chunk + nf - 1) / nf) * nf;   // whole items (tile: half-tiles of 8 frames) per chunk
        per_cu = gen ? (gen_wave ? (fused_prefilter ? p->resident_blocks_gen_pre : p->resident_blocks_gen_wave) : p->resident_blocks_gen)
                     : (pair ? p->resident_blocks_pair : (row ? p->resident_blocks_row : (tile ? p->resident_blocks : p->resident_blocks_frame)));
    }
    dsp::SpanRing::Lease slot;
    if (rg) {
        const int rc = ragged_mfcc_spans(p, *rg, n_frames, a.chunk, slot, st);
        if (rc < 0) return rc;
        a.spans = static_cast<const dsp::ClipSpan *>(slot.d());
        a.n_clips = rg->n_spans;
    }
    const int blocks = grid(p, per_cu, (n_frames + a.chunk - 1) / a.chunk);
    if (fused_prefilter && !(gen_wave && p->d_scan)) return fail(DSP_EINVAL, "internal: fused prefilter without its tables");
    auto launch = [&](const dsp::Mfcc512Args &x) {
        if (fft2048) return dsp::launch_mfcc2048(x, p->d_tables2048, blocks, st, false);
        if (x.log_mode == DSP_LOG_GLOBAL_REF1)      // the wave-per-frame kernel's per-frame epilogue
            return dsp::launch_mfcc512(x, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st, false);
        if (gen_wave) return dsp::launch_mfcc1024_wave(x, p->d_gen_tables, blocks, st, fused_prefilter ? p->d_scan : nullptr, p->scan_steps);
        if (gen) return dsp::launch_mfcc1024(x, p->d_gen_tables, blocks, st);
#ifdef DSP_AMD_EXPERIMENTS
        if (pair) return dsp::launch_mfcc512_pair(x, p->d_pair, blocks, st);
        if (row) return dsp::launch_mfcc512_row(x, p->d_row_tables, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st);
#endif
        return dsp::launch_mfcc512(x, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st, tile);
    };
    if (a.log_mode == DSP_LOG_GLOBAL_REF1 && clip_mode) return two_pass_floor(p, a, st, launch);
    DSP_HIP(launch(a));      // (DSP_LOG_GLOBAL_REF1 on independent frames: one pass, every frame its own clip)
    return DSP_OK;
}

extern "C" {

int dsp_mfcc_frames_device(dsp_mfcc_plan *p, const float *d_frames, long n_frames, float *d_out, void *stream)
{
    if (!p || n_frames < 0 || (n_frames > 0 && (!d_frames || !d_out))) return fail(DSP_EINVAL, "bad argument");
    if (p->cfg.prefilter == DSP_PREFILTER_NONE) return run(p, d_frames, d_out, n_frames, 0, 0, stream);
    // BASELINE config 3: 8th-order Butterworth (donut-classifier/classifier.c:420-446, float64) over each
    // frame from zero state, rounded to float, then the MFCC chain.
    // One pass (1024-sample frames on the wave kernel, 16-byte aligned input): the filter runs inside the MFCC kernel as a
    // float64 parallel-form scan over the wave's lanes -- the frame is read once, nothing filtered is written.  This entry
    // point is tolerance-gated (1e-4 of the frame's L-inf norm); the scan equals the serial recurrence to ~1e-13 before the
    // rounding to float.  dsp_butter_bandpass_filter_* keep the bit-exact serial recurrence.
    if (p->d_scan && p->kernel != DSP_KERNEL_ROW && (reinterpret_cast<uintptr_t>(d_frames) & 15) == 0 && !std::getenv("DSP_AMD_PREFILTER_TWO_PASS"))
        return run(p, d_frames, d_out, n_frames, 0, 0, stream, 0, true);
    // Otherwise two passes: filtered frames go through a bounded workspace (sub-batches of <= 1 Mi frames).
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_ON_DEVICE(p->device);
    const int fl = p->cfg.frame_length;
    const long sub = std::min<long>(n_frames, 1L << 20);
    DSP_HIP(p->d_filtered.reserve((size_t)sub * fl * sizeof(float)));
    dsp::IirCoefD c;
    dsp_butter_bandpass(p->cfg.prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 1000 : 3000,
                        p->cfg.prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 3000 : 7500, c.b, c.a);
    for (long f0 = 0; f0 < n_frames; f0 += sub) {
        const long cnt = std::min(sub, n_frames - f0);
        DSP_HIP(dsp::launch_iir_f64_on_f32(d_frames + f0 * fl, cnt, fl, fl, c, p->d_filtered, (hipStream_t)stream));
        const int rc = run(p, p->d_filtered, d_out + f0 * p->cfg.n_mfcc, cnt, 0, 0, stream);
        if (rc < 0) return rc;
    }
    return DSP_OK;
}

int dsp_mfcc_clips_device(dsp_mfcc_plan *p, const float *d_signal, long n_clips, int samples_per_clip,
                          long clip_stride, float *d_out, int max_frames, void *stream)
{
    if (!p || n_clips < 0) return fail(DSP_EINVAL, "bad argument");
    if (p->cfg.prefilter != DSP_PREFILTER_NONE) return fail(DSP_EINVAL, "the per-frame prefilter applies to independent frames only");
    const int t = dsp_mfcc_frames_for(&p->cfg, samples_per_clip, max_frames);
    if (t == 0 || n_clips == 0) return 0;
    if (!d_signal || !d_out) return fail(DSP_EINVAL, "NULL buffer");
    if (n_clips > 1 && clip_stride < samples_per_clip) return fail(DSP_EINVAL, "clip_stride < samples_per_clip");
    const int rc = run(p, d_signal, d_out, n_clips * (long)t, t, clip_stride, stream, 0, false, samples_per_clip);
    return rc < 0 ? rc : t;
}

int dsp_mfcc_clips_pcm16_device(dsp_mfcc_plan *p, const int16_t *d_pcm, long n_clips, int samples_per_clip,
                                long clip_stride, int channels, int stereo_mode, float *d_out, int max_frames, void *stream)
{
    const int kind = dsp::pcm16_kind(channels, stereo_mode);
    if (kind < 0) return kind;
    if (!p || n_clips < 0) return fail(DSP_EINVAL, "bad argument");
    if (p->cfg.prefilter != DSP_PREFILTER_NONE) return fail(DSP_EINVAL, "the per-frame prefilter applies to independent float frames only");
    const int t = dsp_mfcc_frames_for(&p->cfg, samples_per_clip, max_frames);
    if (t == 0 || n_clips == 0) return 0;
    if (!d_pcm || !d_out) return fail(DSP_EINVAL, "NULL buffer");
    if (n_clips > 1 && clip_stride < samples_per_clip) return fail(DSP_EINVAL, "clip_stride < samples_per_clip");
    const int rc = run(p, d_pcm, d_out, n_clips * (long)t, t, clip_stride, stream, kind, false, samples_per_clip);
    return rc < 0 ? rc : t;
}

// ---- ragged MFCC matrices: clips of different lengths in one launch, their matrices back to back ----

// host only: frame_offsets[c + 1] = frame_offsets[c] + the frames of clip c; the total, or < 0 (offsets not non-decreasing).  lengths: clip c
// is samples [offsets[c], offsets[c] + lengths[c]) instead (RaggedBatch)
static long ragged_frame_offsets(const dsp_mfcc_config &cfg, const long *offsets, long n_clips, int max_frames, long *frame_offsets, int *t_max,
                                 const long *lengths = nullptr)
{
    frame_offsets[0] = 0;
    int tm = 0;
    for (long c = 0; c < n_clips; ++c) {
        const long n = lengths ? (offsets[c] >= 0 && lengths[c] >= 0 && lengths[c] <= INT32_MAX ? lengths[c] : fail(DSP_EINVAL, "internal: bad span"))
                               : dsp::ragged_clip_length(offsets, c);
        if (n < 0) return n;
        const int t = dsp_mfcc_frames_for(&cfg, (int)n, max_frames);
        frame_offsets[c + 1] = frame_offsets[c] + t;
        tm = std::max(tm, t);
    }
    if (t_max) *t_max = tm;
    return frame_offsets[n_clips];
}

long dsp_mfcc_ragged_frame_offsets(const dsp_mfcc_config *cfg, const long *offsets, long n_clips, int max_frames, long *frame_offsets)
{
    if (!cfg || !offsets || !frame_offsets || n_clips < 0) return fail(DSP_EINVAL, "bad argument (cfg, offsets, frame_offsets non-NULL, n_clips >= 0)");
    std::string why;
    if (!valid_cfg(*cfg, why)) return fail(DSP_EINVAL, why);
    return ragged_frame_offsets(*cfg, offsets, n_clips, max_frames, frame_offsets, nullptr);
}

// in_kind as run(); returns the frames of the longest clip.  lengths: spans [offsets[c], offsets[c] + lengths[c]) (RaggedBatch)
static int mfcc_clips_ragged(dsp_mfcc_plan *p, const void *d_in, int in_kind, long n_clips, const long *offsets, int max_frames, float *d_out,
                             void *stream, const long *lengths = nullptr)
{
    if (in_kind < 0) return in_kind;
    if (!p || n_clips < 0 || !offsets) return fail(DSP_EINVAL, "bad argument");
    if (p->cfg.prefilter != DSP_PREFILTER_NONE) return fail(DSP_EINVAL, "ragged MFCC matrices: prefilter plans are not supported (the per-frame prefilter applies to independent frames)");
    if (p->cfg.n_fft == 1024) return fail(DSP_EINVAL, "ragged MFCC matrices run on the 512- and 2048-point kernels: n_fft 1024 is not supported");
    if (p->cfg.n_fft == 512 && p->kernel != DSP_KERNEL_WAVE && p->kernel != DSP_KERNEL_WAVE_FRAME)
        return fail(DSP_EINVAL, "ragged MFCC matrices run on the wave-per-frame kernels (DSP_KERNEL_WAVE / DSP_KERNEL_WAVE_FRAME)");
    if (n_clips >= (1L << 31)) return fail(DSP_EINVAL, "too many clips");
    std::vector<long> fo((size_t)n_clips + 1);
    int t_max = 0;
    const long total = ragged_frame_offsets(p->cfg, offsets, n_clips, max_frames, fo.data(), &t_max, lengths);
    if (total < 0) return (int)total;
    if (total == 0) return 0;
    if (!d_in || !d_out) return fail(DSP_EINVAL, "NULL buffer");
    RaggedBatch rg{offsets, fo.data(), n_clips, 0, lengths};
    for (long c = 0; c < n_clips; ++c) rg.n_spans += fo[(size_t)c + 1] > fo[(size_t)c];
    const int rc = run(p, d_in, d_out, total, 0, 0, stream, in_kind, false, 0, &rg);
    return rc < 0 ? rc : t_max;
}

int dsp_mfcc_clips_ragged_device(dsp_mfcc_plan *p, const float *d_signal, long n_clips, const long *offsets, int max_frames, float *d_out, void *stream)
{
    return mfcc_clips_ragged(p, d_signal, 0, n_clips, offsets, max_frames, d_out, stream);
}

int dsp_mfcc_clips_ragged_pcm16_device(dsp_mfcc_plan *p, const int16_t *d_pcm, long n_clips, const long *offsets, int channels, int stereo_mode,
                                       int max_frames, float *d_out, void *stream)
{
    return mfcc_clips_ragged(p, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, max_frames, d_out, stream);
}

int dsp_mfcc_frames_host(dsp_mfcc_plan *p, const float *frames, long n_frames, float *out)
{
    if (!p || n_frames < 0 || (n_frames > 0 && (!frames || !out))) return fail(DSP_EINVAL, "bad argument");
    if (n_frames == 0) return DSP_OK;
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_ON_DEVICE(p->device);
    const size_t in_b = (size_t)n_frames * p->cfg.frame_length * sizeof(float);
    const size_t out_b = (size_t)n_frames * p->cfg.n_mfcc * sizeof(float);
    DSP_HIP(p->d_in.reserve(in_b));
    DSP_HIP(p->d_out.reserve(out_b));
    int rc;
    DSP_HIP(hipMemcpyAsync(p->d_in, frames, in_b, hipMemcpyHostToDevice, nullptr));
    if (p->cfg.prefilter != DSP_PREFILTER_NONE) return fail(DSP_EINVAL, "prefiltered plans take device buffers (dsp_mfcc_frames_device)");
    if ((rc = run(p, p->d_in, p->d_out, n_frames, 0, 0, nullptr)) < 0) return rc;
    DSP_HIP(hipMemcpyAsync(out, p->d_out, out_b, hipMemcpyDeviceToHost, nullptr));
    DSP_HIP(hipStreamSynchronize(nullptr));
    return DSP_OK;
}

int dsp_mfcc_clips_host(dsp_mfcc_plan *p, const float *signal, long n_clips, int samples_per_clip,
                        long clip_stride, float *out, int max_frames)
{
    if (!p || n_clips < 0) return fail(DSP_EINVAL, "bad argument");
    const int t = dsp_mfcc_frames_for(&p->cfg, samples_per_clip, max_frames);
    if (t == 0 || n_clips == 0) return 0;
    if (!signal || !out) return fail(DSP_EINVAL, "NULL buffer");
    if (n_clips > 1 && clip_stride < samples_per_clip) return fail(DSP_EINVAL, "clip_stride < samples_per_clip");
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_ON_DEVICE(p->device);
    // device copy is packed with an even stride so every frame start stays 8-byte aligned
    const long dstride = samples_per_clip + (samples_per_clip & 1);
    const size_t in_b = (size_t)n_clips * dstride * sizeof(float);
    const size_t out_b = (size_t)n_clips * t * p->cfg.n_mfcc * sizeof(float);
    DSP_HIP(p->d_in.reserve(in_b));
    DSP_HIP(p->d_out.reserve(out_b));
    int rc;
    DSP_HIP(hipMemcpy2DAsync(p->d_in, dstride * sizeof(float), signal, clip_stride * sizeof(float),
                             (size_t)samples_per_clip * sizeof(float), (size_t)n_clips, hipMemcpyHostToDevice, nullptr));
    if ((rc = run(p, p->d_in, p->d_out, n_clips * (long)t, t, dstride, nullptr, 0, false, samples_per_clip)) < 0) return rc;
    DSP_HIP(hipMemcpyAsync(out, p->d_out, out_b, hipMemcpyDeviceToHost, nullptr));
    DSP_HIP(hipStreamSynchronize(nullptr));
    return t;
}

#ifdef DSP_PF_STAMPS
__attribute__((visibility("default"))) int dsp_debug_pf_stamps(unsigned long long *out, int count)     // tools/pf_stamps.py
{
    DSP_HIP(hipDeviceSynchronize());
    DSP_HIP(dsp::read_pf_stamps(out, count));
    return DSP_OK;
}
#endif
#ifdef DSP_RC_STAMPS
__attribute__((visibility("default"))) int dsp_debug_rc_stamps(unsigned long long *out, int count)     // diagnostic builds only (tools/rc_stamps.py)
{
    DSP_HIP(hipDeviceSynchronize());
    DSP_HIP(dsp::read_rc_stamps(out, count));
    return DSP_OK;
}
__attribute__((visibility("default"))) int dsp_debug_bd_stamps(unsigned long long *out, int count)
{
    DSP_HIP(hipDeviceSynchronize());
    DSP_HIP(dsp::read_bd_stamps(out, count));
    return DSP_OK;
}
#endif

}  // extern "C"

// ---- pooling + SVM ---------------------------------------------------------------------

struct dsp_svm {
    int device = 0;
    dsp::SvmModelDev m{};
    dsp::DeviceBuf<float> d_blob;
    dsp::SpanRing scan;      // dsp_svm_scan_device: the per-recording arrays on their way to the GPU (capi_util.hpp)
};

extern "C" {

int dsp_mfcc_stats_device(const float *d_mfcc, long n_clips, int n_frames, int n_coef, float *d_feat, void *stream)
{
    if (n_clips < 0 || n_frames <= 0 || n_coef <= 0 || n_coef > 64 || (n_clips > 0 && (!d_mfcc || !d_feat)))
        return fail(DSP_EINVAL, "bad argument");
    if (n_clips == 0) return DSP_OK;
    // no handle here: launch on the GPU the caller's buffer lives on
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_mfcc) != hipSuccess || attr.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(DSP_EINVAL, "d_mfcc is not a device pointer");
    }
    DSP_ON_DEVICE(attr.device);
    DSP_HIP(dsp::launch_mfcc_stats(d_mfcc, n_clips, n_frames, n_coef, d_feat, (hipStream_t)stream));
    return DSP_OK;
}

int dsp_svm_create(int device, int n_features, int n_sv, const float *offset, const float *scale,
                   const float *support_vectors, const float *coefficients, float gamma, float rho, float prob_a,
                   float prob_b, dsp_svm **out)
{
    if (!out || !offset || !scale || !support_vectors || !coefficients || n_features <= 0 || n_features > 256 || n_sv <= 0)
        return fail(DSP_EINVAL, "bad argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(DSP_ENODEV, "no HIP device: libdsp_amd has no CPU fallback");
    if (device < 0 || device >= n) return fail(DSP_EINVAL, "device index out of range");
    DSP_ON_DEVICE(device);
    auto s = std::make_unique<dsp_svm>();
    s->device = device;
    const size_t nf = n_features, ns = n_sv, total = 2 * nf + ns * nf + ns;
    if (s->d_blob.alloc(total * sizeof(float)) != hipSuccess) return fail(DSP_ENOMEM, "hipMalloc");
    float *p = s->d_blob;
    hipError_t e = hipMemcpy(p, offset, nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p + nf, scale, nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p + 2 * nf, support_vectors, ns * nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p + 2 * nf + ns * nf, coefficients, ns * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(DSP_EHIP, hipGetErrorString(e));
    s->m = {n_features, n_sv, gamma, rho, prob_a, prob_b, p, p + nf, p + 2 * nf, p + 2 * nf + ns * nf};
    *out = s.release();
    return DSP_OK;
}

void dsp_svm_destroy(dsp_svm *s)
{
    if (!s) return;
    dsp::DeviceScope dsp_device_scope_(s->device);
    s->scan.release();
    delete s;
}

}  // extern "C"

// Ragged batch -> spans in a ring slot (uploaded on `stream`).  offsets[n_clips + 1]: clip c is samples [offsets[c], offsets[c + 1]) per
// channel of the buffer; every clip must hold at least one frame.  *t_max: frames of the longest clip.
// The kernels deal the spans to their n_waves wavefronts in fixed order (wave w walks spans w, w + n_waves, ...), so the ORDER of the
// spans is the load balance: by frame count, longest first, and snaking -- left to right over the waves in even rounds, right to left in
// odd ones -- every wave's total is within a clip of the mean (in the caller's order: +14 % on clips of 0.5 - 1.5 s).
// (host only: no HIP call) fills h[n_clips]; returns DSP_OK or DSP_EINVAL with the reason
static int build_fused_spans(const dsp_mfcc_config &cfg, const long *offsets, long n_clips, int max_frames, long n_waves, dsp::ClipSpan *h, int *t_max)
{
    std::vector<int> frames((size_t)n_clips), order((size_t)n_clips);
    int tm = 0;
    for (long c = 0; c < n_clips; ++c) {
        const long n = dsp::ragged_clip_length(offsets, c);
        if (n < 0) return (int)n;
        const int t = dsp_mfcc_frames_for(&cfg, (int)n, max_frames);
        if (t == 0) return fail(DSP_EINVAL, "clip " + std::to_string(c) + " of the ragged batch is shorter than one frame");
        frames[c] = t;
        tm = std::max(tm, t);
    }
    dsp::order_by_key_desc(frames.data(), n_clips, tm, order.data());
    n_waves = std::max(1L, n_waves);
    for (long i = 0; i < n_clips; ++i) {
        const long round = i / n_waves, j = i - round * n_waves;
        const long width = std::min(n_waves, n_clips - round * n_waves);          // the last round may be short
        const long pos = round * n_waves + ((round & 1) ? width - 1 - j : j);
        const long c = order[i];
        h[pos] = dsp::ClipSpan{offsets[c], (int)(offsets[c + 1] - offsets[c]), frames[c], c, 0};
    }
    *t_max = tm;
    return DSP_OK;
}

// the fused kernels' spans in the leased ring slot, uploaded on st
static int ragged_spans(dsp_mfcc_plan *p, const long *offsets, long n_clips, int max_frames, long n_waves, dsp::SpanRing::Lease &slot, int *t_max, hipStream_t st)
{
    if (!offsets) return fail(DSP_EINVAL, "offsets is NULL");
    if (n_clips >= (1L << 31)) return fail(DSP_EINVAL, "too many clips");
    DSP_HIP(p->spans.acquire((size_t)n_clips * sizeof(dsp::ClipSpan), slot));
    const int rc = build_fused_spans(p->cfg, offsets, n_clips, max_frames, n_waves, static_cast<dsp::ClipSpan *>(slot.h()), t_max);
    if (rc < 0) return rc;
    DSP_HIP(slot.upload((size_t)n_clips * sizeof(dsp::ClipSpan), st));
    return DSP_OK;
}

/* Test hook (host only): the order a ragged batch of the fused clip kernels runs in -- spans[pos] = {start, samples, frames, caller's
 * index} as 4 longs per clip; wave w of n_waves walks pos = w, w + n_waves, ...  tests/test_capi_cpu.py checks it (also under ASan). */
extern "C" int dsp_debug_fused_spans(const dsp_mfcc_config *cfg, const long *offsets, long n_clips, int max_frames, long n_waves, long *out4)
{
    if (!cfg || !offsets || n_clips < 0 || (n_clips > 0 && !out4)) return fail(DSP_EINVAL, "bad argument");
    std::vector<dsp::ClipSpan> h((size_t)n_clips);
    int tm = 0;
    const int rc = build_fused_spans(*cfg, offsets, n_clips, max_frames, n_waves, h.data(), &tm);
    if (rc < 0) return rc;
    for (long i = 0; i < n_clips; ++i) { out4[4 * i] = h[i].off; out4[4 * i + 1] = h[i].n; out4[4 * i + 2] = h[i].frames; out4[4 * i + 3] = h[i].orig; }
    return tm;
}

// clip -> label in one kernel; in_kind 0 = float samples, 1 / 2 / 3 = int16 mono / stereo channel 0 / stereo average.
// offsets != nullptr: a ragged batch (clips of different lengths back to back or anywhere in the buffer; samples_per_clip / clip_stride unused)
static int scrubjay_fused(dsp_mfcc_plan *p, dsp_svm *s, const void *d_signal, int in_kind, long n_clips, int samples_per_clip,
                          long clip_stride, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream,
                          const long *offsets = nullptr)
{
    if (in_kind < 0) return in_kind;
    if (!p || !s || n_clips < 0) return fail(DSP_EINVAL, "bad argument");
    if ((p->cfg.n_fft != 512 && p->cfg.n_fft != 2048) || (p->cfg.log_mode != DSP_LOG_PER_FRAME_MAX && p->cfg.log_mode != DSP_LOG_LOG10_FLOOR) ||
        p->cfg.prefilter != DSP_PREFILTER_NONE || p->kernel != DSP_KERNEL_WAVE)
        return fail(DSP_EINVAL, "the fused clip -> label path runs on the 512- and 2048-point wave-per-frame kernels, per-frame log modes");
    if (in_kind != 0 && !p->aub && (p->cfg.n_fft != 512 || p->cfg.frame_length != 400 || p->host.mel_gather != 3 ||
                                     !((p->host.dct_split == 4 && p->host.dct_len == 10) || (p->host.dct_split == 2 && p->host.dct_len == 20))))
        return fail(DSP_EINVAL, "int16 input of the fused clip -> label kernel: the reference framing (n_fft 512, frame 400, 40 mel filters, up to 20 coefficients) "
                                "or the scrubjay_infer.c front end (dsp_mfcc_scrubjay_infer_config)");
    if (s->m.n_features != 2 * p->cfg.n_mfcc || s->m.n_features > 64) return fail(DSP_EINVAL, "SVM n_features must equal 2 * n_mfcc (<= 64)");
    if (p->cfg.n_fft == 512 && s->m.n_sv > dsp::kSvmFused512MaxSv)
        return fail(DSP_EINVAL, "the 512-point fused clip -> label kernel holds at most " + std::to_string(dsp::kSvmFused512MaxSv) +
                                " support vectors in LDS (this SVM has " + std::to_string(s->m.n_sv) + "): use the three calls");
    const bool ragged = offsets != nullptr;
    int t = ragged ? 1 : dsp_mfcc_frames_for(&p->cfg, samples_per_clip, max_frames);
    if (n_clips == 0) return 0;
    if (t == 0) return fail(DSP_EINVAL, "clips shorter than one frame have no features to pool");
    if (!d_signal || !d_labels) return fail(DSP_EINVAL, "NULL buffer");
    if (!ragged && n_clips > 1 && clip_stride < samples_per_clip) return fail(DSP_EINVAL, "clip_stride < samples_per_clip");
    if ((reinterpret_cast<uintptr_t>(d_signal) & (in_kind == 1 ? 3 : 7)) || (!ragged && n_clips > 1 && (clip_stride & 1)))
        return fail(DSP_EINVAL, "input must be 8-byte aligned (4 for mono int16) with an even clip stride");
    if (s->device != p->device) return fail(DSP_EINVAL, "plan and SVM live on different devices");
    DSP_ON_DEVICE(p->device);
    hipStream_t st = (hipStream_t)stream;
    const int blocks = grid(p, p->cfg.n_fft == 2048 ? p->resident_blocks_2048_pool : p->resident_blocks, n_clips);
    dsp::SpanRing::Lease slot;
    if (ragged) {
        const int rc = ragged_spans(p, offsets, n_clips, max_frames, 4L * blocks, slot, &t, st);
        if (rc < 0) return rc;
    }
    dsp::Mfcc512Args a = plan_args(p, d_signal, in_kind, true);
    a.n_frames = n_clips * (long)t;
    a.n_clips = n_clips;
    a.spans = ragged ? static_cast<const dsp::ClipSpan *>(slot.d()) : nullptr;
    a.clip_stride = ragged ? 0 : clip_stride;
    a.frames_per_clip = t;
    a.chunk = t;                                  // one wavefront walks one clip
    a.samples_per_clip = ragged ? 0 : samples_per_clip;
    a.pool = dsp::PoolSvmArgs{s->m, d_labels, d_decision, d_prob1, d_feat};
    if (p->cfg.n_fft == 2048)      // scrubjay_infer.c's own framing (WIN_SIZE 2048, HOP_SIZE 1024): mfcc2048_kernel<POOL>
        DSP_HIP(dsp::launch_mfcc2048(a, p->d_tables2048, blocks, st, true));
    else
        DSP_HIP(dsp::launch_mfcc512_pool(a, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st));
    return t;
}

extern "C" {

int dsp_scrubjay_fused_device(dsp_mfcc_plan *p, dsp_svm *s, const float *d_signal, long n_clips, int samples_per_clip,
                              long clip_stride, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat,
                              void *stream)
{
    return scrubjay_fused(p, s, d_signal, 0, n_clips, samples_per_clip, clip_stride, max_frames, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_fused_pcm16_device(dsp_mfcc_plan *p, dsp_svm *s, const int16_t *d_pcm, long n_clips, int samples_per_clip, long clip_stride,
                                    int channels, int stereo_mode, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat,
                                    void *stream)
{
    return scrubjay_fused(p, s, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, samples_per_clip, clip_stride, max_frames, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_fused_ragged_device(dsp_mfcc_plan *p, dsp_svm *s, const float *d_signal, long n_clips, const long *offsets, int max_frames,
                                     int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    if (!offsets) return fail(DSP_EINVAL, "offsets is NULL");
    return scrubjay_fused(p, s, d_signal, 0, n_clips, 0, 0, max_frames, d_labels, d_decision, d_prob1, d_feat, stream, offsets);
}

int dsp_scrubjay_fused_ragged_pcm16_device(dsp_mfcc_plan *p, dsp_svm *s, const int16_t *d_pcm, long n_clips, const long *offsets, int channels,
                                           int stereo_mode, int max_frames, int *d_labels, float *d_decision, float *d_prob1, float *d_feat,
                                           void *stream)
{
    if (!offsets) return fail(DSP_EINVAL, "offsets is NULL");
    return scrubjay_fused(p, s, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, 0, 0, max_frames, d_labels, d_decision, d_prob1, d_feat, stream, offsets);
}

}  // extern "C"

int dsp::plan_device(const dsp_mfcc_plan *plan) { return plan ? plan->device : -1; }

// capi_util.hpp: the ragged MFCC path over spans given by start and length (capi_stream.cpp: one span per stream with new rows)
int dsp::mfcc_spans_device(dsp_mfcc_plan *p, const void *d_in, int in_kind, long n_spans, const long *starts, const long *lengths, float *d_out,
                           void *stream)
{
    if (!lengths) return fail(DSP_EINVAL, "internal: spans without lengths");
    if (p && in_kind > 0 && (p->cfg.n_fft != 512 || p->kernel != DSP_KERNEL_WAVE || p->cfg.log_mode != DSP_LOG_PER_FRAME_MAX))     // as run() would, before any launch
        return fail(DSP_EINVAL, "PCM16 ingestion runs on the 512-point wave-per-frame kernel (per-frame log mode) and on the 2048-point scrubjay_infer.c front end");
    return mfcc_clips_ragged(p, d_in, in_kind, n_spans, starts, INT_MAX, d_out, stream, lengths);
}

// capi_util.hpp: the fused form of dsp_classify_signal_batch_device (capi_consumers.cpp)
int dsp::stop_fused_device(dsp_mfcc_plan *p, const dsp::StopModelDev &m, const void *d_signal, long n_clips, long clip_stride, int t,
                           float *d_prob, void *stream, int in_kind, const long *offsets)
{
    const bool ragged = offsets != nullptr;
    if (ragged) { t = 1; clip_stride = 0; }
    // the reference's shape on the default kernel: 512-point, per-frame log, 13 coefficients of 40 mel energies, complete frames
    if (p->cfg.n_fft != 512 || p->cfg.log_mode != DSP_LOG_PER_FRAME_MAX || p->cfg.prefilter != DSP_PREFILTER_NONE || p->kernel != DSP_KERNEL_WAVE ||
        p->host.dct_split != 4 || p->host.dct_len != 10 || m.n_coef != p->cfg.n_mfcc || m.units[0] > dsp::kStopFusedUnits || !m.fold_a || t <= 0 ||
        std::getenv("DSP_AMD_STOP_TWO_KERNELS"))
        return 0;
    if ((reinterpret_cast<uintptr_t>(d_signal) & (in_kind == 1 ? 3 : 7)) || (n_clips > 1 && (clip_stride & 1))) return 0;      // the two-kernel path reports it
    if (in_kind != 0 && (p->host.mel_gather != 3 || p->cfg.frame_length != 400)) return 0;
    if (m.max_frames <= 0) return fail(DSP_EINVAL, "stop model without frames");
    DSP_ON_DEVICE(p->device);
    hipStream_t st = (hipStream_t)stream;
    const int blocks = dsp::mfcc512_stop_grid(grid(p, p->resident_blocks, n_clips), m, in_kind, p->host.mel_gather, p->cfg.frame_length);      // what the launcher will start
    dsp::SpanRing::Lease slot;
    if (ragged) {      // frames past the model's max_frames are dropped (stop_detector.c:26-30): a clip's walk ends there
        const int rc = ragged_spans(p, offsets, n_clips, m.max_frames, 4L * blocks, slot, &t, st);
        if (rc < 0) return rc;
    }
    dsp::Mfcc512Args a = plan_args(p, d_signal, in_kind, true);
    a.n_frames = n_clips * (long)t;
    a.n_clips = n_clips;
    a.spans = ragged ? static_cast<const dsp::ClipSpan *>(slot.d()) : nullptr;
    a.clip_stride = clip_stride;
    a.frames_per_clip = t;
    a.chunk = t;                                  // one wavefront walks one clip
    a.stop = dsp::StopNetArgs{m, d_prob};
    DSP_HIP(dsp::launch_mfcc512_stop(a, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st));
    return 1;
}

extern "C" {

int dsp_svm_predict_device(dsp_svm *s, const float *d_feat, long n_clips, int *d_labels, float *d_decision,
                           float *d_prob1, void *stream)
{
    if (!s || n_clips < 0 || (n_clips > 0 && (!d_feat || !d_labels))) return fail(DSP_EINVAL, "bad argument");
    DSP_ON_DEVICE(s->device);
    DSP_HIP(dsp::launch_svm_predict(s->m, d_feat, n_clips, d_labels, d_decision, d_prob1, (hipStream_t)stream));
    return DSP_OK;
}

}  // extern "C"

// ---- window scans of long recordings with the SVM: label, decision, P(label 1) and the pooled features per sliding window ------------
// Windows are runs of MFCC rows (capi_util.hpp scan_plan).  Under complete framing and a per-frame log a row depends on its own samples
// only, so a window's rows are rows of the recording's matrix.  Under DSP_FRAMING_STREAM the first H = ceil((frame_length - hop_length) /
// hop_length) rows of a cut-out window see zeros before the window where the recording's rows see samples: each window gets its own
// head rows, from internal spans [start, start + min(H, rows) hop) of the recording (RaggedBatch with lengths).

// the first rows of a stream-framed clip that reach before it (0 under complete framing)
static int head_rows_of(const dsp_mfcc_config &c)
{
    return c.framing == DSP_FRAMING_STREAM ? (c.frame_length - c.hop_length + c.hop_length - 1) / c.hop_length : 0;
}

// host only: window g's clip in samples (absolute in the buffer), or with head_rows > 0 its head span; starts / lengths may be NULL.
// Returns the window count or < 0.
static long window_spans(const dsp_mfcc_config &c, const dsp_scan_config &sc, const long *offsets, long n, long *starts, long *lengths, int head_rows)
{
    const long wf = sc.window_frames, hf = sc.hop_frames, hop = c.hop_length;
    long g = 0;
    for (long r = 0; r < n; ++r) {
        const long len = dsp::ragged_clip_length(offsets, r);
        if (len < 0) return len;
        const long rows = dsp_mfcc_frames_for(&c, (int)len, INT_MAX);
        const long w_n = rows >= wf ? 1 + (rows - wf) / hf : 1;
        const long span = head_rows > 0 ? std::min<long>(head_rows, std::min(rows, wf)) * hop
                                        : (c.framing == DSP_FRAMING_STREAM ? wf * hop : c.frame_length + (wf - 1) * hop);
        for (long w = 0; w < w_n; ++w, ++g) {
            const long a = w * hf * hop;
            if (starts) starts[g] = offsets[r] + a;
            if (lengths) lengths[g] = std::min(span, len - a);
        }
    }
    return g;
}

// dsp_svm_scan_device and the scanner: head_rows > 0 adds window g's head rows, rows [ho[r] + w hc, + hc) of d_head (ho: n + 1 HOST longs)
static int svm_scan(dsp_svm *s, const float *d_mfcc, long n, const long *frame_offsets, const dsp_scan_config *cfg, const float *d_head, int head_rows,
                    const long *ho, int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    if (!s) return fail(DSP_EINVAL, "SVM is NULL");
    long rc = dsp::scan_args(cfg, n);
    if (rc < 0 || n == 0) return (int)rc;
    if (!frame_offsets || !d_mfcc || !d_labels) return fail(DSP_EINVAL, "frame_offsets, d_mfcc and d_labels must not be NULL");
    if ((s->m.n_features & 1) || s->m.n_features > 128) return fail(DSP_EINVAL, "the scan pools n_features / 2 <= 64 coefficients per row: n_features must be even, <= 128");
    const int tw = dsp::svm_scan_tile(s->m.n_features, cfg->window_frames, cfg->hop_frames, head_rows);
    std::vector<long> wo((size_t)n + 1), to((size_t)n + 1);
    if ((rc = dsp::scan_plan(cfg, frame_offsets, n, wo.data(), to.data(), std::max(tw, 1))) < 0) return (int)rc;
    for (long r = 0; r < n; ++r)
        if (frame_offsets[r + 1] == frame_offsets[r])
            return fail(DSP_EINVAL, "recording " + std::to_string(r) + " has no MFCC rows (mfcc_stats pools a window's rows: scrubjay_infer.c:55-59)");
    DSP_ON_DEVICE(s->device);
    dsp::SpanRing::Lease slot;
    DSP_HIP(dsp::scan_upload(s->scan, frame_offsets, n, wo.data(), to.data(), slot, stream, head_rows > 0 ? ho : nullptr));
    const long *d = static_cast<const long *>(slot.d());
    DSP_HIP(dsp::launch_svm_scan(s->m, d_mfcc + frame_offsets[0] * (s->m.n_features / 2), d_head, n, d, d + (n + 1), d + 2 * (n + 1),
                                 head_rows > 0 ? d + 3 * (n + 1) : nullptr, to[(size_t)n], cfg->window_frames, cfg->hop_frames, head_rows, tw, d_labels,
                                 d_decision, d_prob1, d_feat, (hipStream_t)stream));
    return DSP_OK;
}

// the plans whose rows do not depend on the window, on the fused clip -> label kernel's front ends (what per-window equality is against)
static int scan_front_end(const dsp_mfcc_plan *p, const dsp_svm *s)
{
    const dsp_mfcc_config &c = p->cfg;
    if (c.log_mode == DSP_LOG_GLOBAL_REF1) return fail(DSP_EINVAL, "DSP_LOG_GLOBAL_REF1 plans cannot be scanned: the top_db floor spans the window");
    if (c.prefilter != DSP_PREFILTER_NONE || c.n_fft == 1024)
        return fail(DSP_EINVAL, "scans run on the ragged MFCC matrix: prefilter plans and n_fft 1024 are not supported");
    if (p->kernel != DSP_KERNEL_WAVE) return fail(DSP_EINVAL, "scans run on the wave-per-frame kernel (DSP_KERNEL_WAVE), as the fused clip -> label path");
    if (s->m.n_features != 2 * c.n_mfcc || s->m.n_features > 64) return fail(DSP_EINVAL, "SVM n_features must equal 2 * n_mfcc (<= 64)");
    if (s->device != p->device) return fail(DSP_EINVAL, "plan and SVM live on different devices");
    return DSP_OK;
}

// A scrub-jay scanner: PCM -> the recordings' ragged MFCC matrix (+ the windows' head rows) in its own workspace -> svm_scan_kernel.
struct dsp_scrubjay_scanner {
    dsp_mfcc_plan *plan = nullptr;
    dsp_svm *svm = nullptr;
    dsp_scan_config cfg{};
    int head_rows = 0;
    dsp::DeviceBuf<float> d_mfcc, d_head;
    std::vector<long> fo, wo, ho, starts, lengths;
    std::mutex mu;
};

static int scrubjay_scanner_run(dsp_scrubjay_scanner *s, const void *d_signal, int in_kind, long n, const long *offsets, int *d_labels, float *d_decision,
                                float *d_prob1, float *d_feat, void *stream)
{
    if (in_kind < 0) return in_kind;
    if (!s || n < 0) return fail(DSP_EINVAL, "bad argument (scanner, n_recordings >= 0)");
    if (n == 0) return DSP_OK;
    if (!offsets || !d_labels) return fail(DSP_EINVAL, "offsets and d_labels must not be NULL");
    if (n >= (1L << 31)) return fail(DSP_EINVAL, "too many recordings");
    if (const int rc = scan_front_end(s->plan, s->svm)) return rc;
    dsp_mfcc_plan *p = s->plan;
    if (in_kind != 0 && !p->aub && !(p->cfg.n_fft == 512 && p->host.dct_split == 4 && p->host.dct_len == 10 && p->host.mel_gather == 3))
        return fail(DSP_EINVAL, "int16 input of the scrub-jay scan: the ragged MFCC matrix takes it on the scrubjay_infer.c front end "
                                "(dsp_mfcc_scrubjay_infer_config) and on the 512-point framing with up to 13 coefficients of 40 mel filters");
    std::lock_guard<std::mutex> lock(s->mu);
    const int nc = p->cfg.n_mfcc;
    s->fo.resize((size_t)n + 1);
    const long rows = ragged_frame_offsets(p->cfg, offsets, n, INT_MAX, s->fo.data(), nullptr);     // no cap: every row of every recording
    if (rows < 0) return (int)rows;
    for (long r = 0; r < n; ++r)
        if (s->fo[(size_t)r + 1] == s->fo[(size_t)r])
            return fail(DSP_EINVAL, "recording " + std::to_string(r) + " is shorter than one frame: mfcc_stats has no rows to pool (scrubjay_infer.c:55-59)");
    if (!d_signal) return fail(DSP_EINVAL, "d_signal is NULL");
    DSP_ON_DEVICE(p->device);
    if (s->d_mfcc.reserve((size_t)rows * nc * sizeof(float)) != hipSuccess) return fail(DSP_ENOMEM, "hipMalloc (scanner MFCC workspace)");
    int rc = mfcc_clips_ragged(p, d_signal, in_kind, n, offsets, INT_MAX, s->d_mfcc, stream);
    if (rc < 0) return rc;
    if (s->head_rows > 0) {
        // window g of recording r: its min(H, rows) head rows at ho[r] + (g - wo[r]) hc_r, computed from its own head span
        s->wo.resize((size_t)n + 1);
        const long n_win = dsp::scan_plan(&s->cfg, s->fo.data(), n, s->wo.data(), nullptr, 1);
        if (n_win < 0) return (int)n_win;
        s->starts.resize((size_t)n_win);
        s->lengths.resize((size_t)n_win);
        if (window_spans(p->cfg, s->cfg, offsets, n, s->starts.data(), s->lengths.data(), s->head_rows) != n_win) return fail(DSP_EINVAL, "internal: head spans");
        s->ho.resize((size_t)n + 1);
        s->ho[0] = 0;
        for (long r = 0; r < n; ++r) {
            const long hc = std::min<long>(s->head_rows, std::min<long>(s->fo[(size_t)r + 1] - s->fo[(size_t)r], s->cfg.window_frames));
            s->ho[(size_t)r + 1] = s->ho[(size_t)r] + (s->wo[(size_t)r + 1] - s->wo[(size_t)r]) * hc;
        }
        if (s->d_head.reserve((size_t)s->ho[(size_t)n] * nc * sizeof(float)) != hipSuccess)
            return fail(DSP_ENOMEM, "hipMalloc (scanner head-row workspace)");
        if ((rc = mfcc_clips_ragged(p, d_signal, in_kind, n_win, s->starts.data(), INT_MAX, s->d_head, stream, s->lengths.data())) < 0) return rc;
    }
    return svm_scan(s->svm, s->d_mfcc, n, s->fo.data(), &s->cfg, s->d_head, s->head_rows, s->ho.data(), d_labels, d_decision, d_prob1, d_feat, stream);
}

extern "C" {

long dsp_scan_window_spans(const dsp_mfcc_config *mfcc, const dsp_scan_config *cfg, const long *offsets, long n_recordings, long *starts, long *lengths)
{
    if (!mfcc) return fail(DSP_EINVAL, "mfcc config is NULL");
    std::string why;
    if (!valid_cfg(*mfcc, why)) return fail(DSP_EINVAL, why);
    if (const int rc = dsp::scan_args(cfg, n_recordings)) return rc;
    if (n_recordings == 0) return 0;
    if (!offsets) return fail(DSP_EINVAL, "offsets is NULL");
    return window_spans(*mfcc, *cfg, offsets, n_recordings, starts, lengths, 0);
}

int dsp_svm_scan_device(dsp_svm *svm, const float *d_mfcc, long n_recordings, const long *frame_offsets, const dsp_scan_config *cfg, int *d_labels,
                        float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    return svm_scan(svm, d_mfcc, n_recordings, frame_offsets, cfg, nullptr, 0, nullptr, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_scanner_create(dsp_mfcc_plan *plan, dsp_svm *svm, const dsp_scan_config *cfg, dsp_scrubjay_scanner **out)
{
    if (!out) return fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (!plan || !svm) return fail(DSP_EINVAL, "plan and SVM must not be NULL");
    if (const int rc = dsp::scan_args(cfg, 0)) return rc;
    if (const int rc = scan_front_end(plan, svm)) return rc;
    auto *s = new dsp_scrubjay_scanner;
    s->plan = plan;
    s->svm = svm;
    s->cfg = *cfg;
    s->head_rows = head_rows_of(plan->cfg);
    *out = s;
    return DSP_OK;
}

void dsp_scrubjay_scanner_destroy(dsp_scrubjay_scanner *s)
{
    if (!s) return;
    dsp::DeviceScope dsp_device_scope_(s->plan->device);
    delete s;
}

int dsp_scrubjay_scanner_run_device(dsp_scrubjay_scanner *s, const float *d_signal, long n_recordings, const long *offsets, int *d_labels,
                                    float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    return scrubjay_scanner_run(s, d_signal, 0, n_recordings, offsets, d_labels, d_decision, d_prob1, d_feat, stream);
}

int dsp_scrubjay_scanner_run_pcm16_device(dsp_scrubjay_scanner *s, const int16_t *d_pcm, long n_recordings, const long *offsets, int channels,
                                          int stereo_mode, int *d_labels, float *d_decision, float *d_prob1, float *d_feat, void *stream)
{
    return scrubjay_scanner_run(s, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_recordings, offsets, d_labels, d_decision, d_prob1, d_feat, stream);
}

}  // extern "C"

// ---- the reference's entry point ------------------------------------------------

static dsp_mfcc_plan *g_default_plan = nullptr;
static std::mutex g_default_mu;

// 2fa/audio/word/c/mfcc.h:16-19.  Same contract as the reference: returns the
// frame count, 0 for "clip too short / no room"; a GPU failure also returns 0
// (no frames were produced) with the cause in dsp_last_error().
extern "C" int compute_mfcc(const float *signal, int num_samples, float *out_mfcc, int max_frames)
{
    dsp_mfcc_config cfg;
    dsp_mfcc_default_config(&cfg);
    if (dsp_mfcc_frames_for(&cfg, num_samples, max_frames) == 0) return 0;   // mfcc.c:117-119
    if (!signal || !out_mfcc) { fail(DSP_EINVAL, "NULL buffer"); return 0; }
    dsp_mfcc_plan *plan;
    {
        std::lock_guard<std::mutex> lock(g_default_mu);
        if (!g_default_plan) {
            const char *dev = std::getenv("DSP_AMD_DEVICE");
            if (dsp_mfcc_plan_create(&cfg, dev ? std::atoi(dev) : 0, &g_default_plan) < 0) {
                std::fprintf(stderr, "libdsp_amd: compute_mfcc: %s\n", dsp_last_error());
                return 0;
            }
        }
        plan = g_default_plan;
    }
    const int t = dsp_mfcc_clips_host(plan, signal, 1, num_samples, num_samples, out_mfcc, max_frames);
    if (t < 0) {
        std::fprintf(stderr, "libdsp_amd: compute_mfcc: %s\n", dsp_last_error());
        return 0;
    }
    return t;
}
