// capi.cpp -- the C ABI of libdsp_amd.so (include/dsp_amd.h): the error sink, configurations and tables, the MFCC plans (mfcc_plan.hpp)
// and their frame / clip / ragged / host entry points, compute_mfcc.  The SVM, the fused clip kernels and the SVM scans are
// capi_scrubjay.cpp, the stop net and the speaker GMM capi_consumers.cpp, stream sessions capi_stream.cpp, the donut classifiers
// capi_classify_f32.cpp and capi_classify_f64.cpp.
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
#include "classify_kernels.hpp"
#include "host_pipe.hpp"
#include "mfcc_plan.hpp"

#ifdef DSP_PF_STAMPS
namespace dsp { hipError_t read_pf_stamps(unsigned long long *host, int count); }      // mfcc_kernels.hip, diagnostic builds
#endif
#ifdef DSP_RC_STAMPS
namespace dsp { hipError_t read_rc_stamps(unsigned long long *host, int count); hipError_t read_bd_stamps(unsigned long long *host, int count); }      // classify_kernels.hip, diagnostic builds
#endif

static thread_local std::string g_err;

// error sink shared with the other translation units of the C ABI (capi_util.hpp)
int dsp::capi_fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

using dsp::capi_fail;
using dsp::mfcc_run;
using dsp::MfccJob;
using dsp::RaggedBatch;
using dsp::valid_cfg;

// n_fft 400 (mfcc400_kernel.hip): librosa.feature.mfcc(n_fft = 400) of gmm_utils.py:52-58 and its neighbours; every refusal names the field
static bool valid_cfg_400(const dsp_mfcc_config &c, std::string &why)
{
    if (c.frame_length != 400) { why = "frame_length must be 400 for n_fft = 400"; return false; }
    if (c.win_length != 0) { why = "win_length must be 0 for n_fft = 400"; return false; }
    if (c.n_mels > dsp::k400MaxMels) { why = "n_mels must be in [1, 128] for n_fft = 400"; return false; }
    if (c.n_mfcc > std::min(c.n_mels, dsp::k400MaxMfcc)) { why = "n_mfcc must be in [1, min(n_mels, 32)] for n_fft = 400"; return false; }
    if (c.mel_norm == DSP_MELNORM_AUBIO_SLANEY) { why = "mel_norm: DSP_MELNORM_AUBIO_SLANEY is implemented for n_fft = 2048"; return false; }
    if (c.log_mode == DSP_LOG_LOG10_FLOOR) { why = "log_mode: DSP_LOG_LOG10_FLOOR is implemented for n_fft = 2048"; return false; }
    if (c.spectrum != DSP_SPECTRUM_POWER) { why = "spectrum: DSP_SPECTRUM_MAGNITUDE is implemented for n_fft = 2048"; return false; }
    if (c.framing == DSP_FRAMING_STREAM) { why = "framing: DSP_FRAMING_STREAM is implemented for n_fft = 2048"; return false; }
    if (c.prefilter != DSP_PREFILTER_NONE) { why = "prefilter: the per-frame prefilter is implemented for n_fft = 512 and 1024"; return false; }
    if (c.fmax > 0.5f * (float)c.sample_rate) { why = "fmax must not exceed sample_rate / 2 for n_fft = 400"; return false; }
    return true;
}

// DSP_FRAMING_CENTER at n_fft 2048 (mfcc2048_kernel.hip, CENTER): librosa.feature.mfcc with librosa's default n_fft, keyword_classifier.py:41-44 and
// cepstrum/train.py:38-40 (dsp_mfcc_librosa_config), on the reference-semantics family of the kernel; every refusal names the field
static bool valid_cfg_2048_center(const dsp_mfcc_config &c, std::string &why)
{
    if (c.frame_length != 2048) { why = "frame_length must be 2048 for DSP_FRAMING_CENTER at n_fft = 2048"; return false; }
    if (c.win_length != 0) { why = "win_length must be 0 for DSP_FRAMING_CENTER at n_fft = 2048"; return false; }
    if (c.n_mels > dsp::k2048MaxMels) { why = "n_mels must be in [1, 128] for n_fft = 2048"; return false; }
    if (c.n_mfcc > dsp::k2048MaxMfcc) { why = "n_mfcc must be in [1, 32] for n_fft = 2048"; return false; }
    if (c.spectrum != DSP_SPECTRUM_POWER) { why = "spectrum: DSP_SPECTRUM_MAGNITUDE is not implemented with DSP_FRAMING_CENTER"; return false; }
    if (c.log_mode == DSP_LOG_LOG10_FLOOR) { why = "log_mode: DSP_LOG_LOG10_FLOOR is not implemented with DSP_FRAMING_CENTER"; return false; }
    if (c.mel_norm == DSP_MELNORM_AUBIO_SLANEY) { why = "mel_norm: DSP_MELNORM_AUBIO_SLANEY is not implemented with DSP_FRAMING_CENTER"; return false; }
    if (c.prefilter != DSP_PREFILTER_NONE) { why = "prefilter: the per-frame prefilter is implemented for n_fft = 512 and 1024"; return false; }
    return true;
}

bool dsp::valid_cfg(const dsp_mfcc_config &c, std::string &why)
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
    if (c.framing != DSP_FRAMING_COMPLETE && c.framing != DSP_FRAMING_STREAM && c.framing != DSP_FRAMING_CENTER) { why = "unknown framing"; return false; }
    if (c.framing == DSP_FRAMING_CENTER && c.n_fft != 400 && c.n_fft != 2048) { why = "framing: DSP_FRAMING_CENTER is implemented for n_fft = 400 and 2048"; return false; }
    if (c.n_fft == 400) return valid_cfg_400(c, why);
    if (c.framing == DSP_FRAMING_CENTER) return valid_cfg_2048_center(c, why);
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
    if (c.n_fft != 512 && c.n_fft != 1024 && c.n_fft != 2048) { why = "n_fft must be 400, 512, 1024 or 2048"; return false; }
    return true;
}

extern "C" {

const char *dsp_last_error(void) { return g_err.c_str(); }
#ifndef DSP_AMD_SRC_HASH
#define DSP_AMD_SRC_HASH "unknown"
#endif
const char *dsp_version(void) { return "dsp_amd 0.3 (gfx950) src:" DSP_AMD_SRC_HASH; }

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

void dsp_mfcc_speaker_config(dsp_mfcc_config *c)
{
    // 2fa/audio/speaker/gmm_utils.py:8-11 (SAMPLE_RATE 16000, N_MFCC 13, N_FFT 400, HOP_LENGTH 160), :52-58 (librosa.feature.mfcc
    // with librosa's defaults for everything else: center = True, 128 Slaney mel filters, power_to_db(ref = 1, top_db = 80))
    dsp_mfcc_default_config(c);
    c->sample_rate = 16000;
    c->n_fft = 400;
    c->frame_length = 400;
    c->hop_length = 160;
    c->n_mels = 128;
    c->n_mfcc = 13;
    c->window = DSP_WINDOW_HANN;
    c->mel_norm = DSP_MELNORM_LIBROSA;
    c->log_mode = DSP_LOG_GLOBAL_REF1;
    c->spectrum = DSP_SPECTRUM_POWER;
    c->framing = DSP_FRAMING_CENTER;
    c->win_length = 0;
    c->prefilter = DSP_PREFILTER_NONE;
    c->fmin = 0.0f;
    c->fmax = 8000.0f;
    c->amin = 1e-10f;
    c->top_db = 80.0f;
}

void dsp_mfcc_librosa_config(dsp_mfcc_config *c, int sample_rate, int n_mfcc)
{
    // 2fa/audio/keyword_classifier.py:41-44 (librosa.feature.mfcc(y, sr = 22050, n_mfcc = 13)) and cepstrum/train.py:38-40, run.py:11-14
    // (n_mfcc = 20), with librosa's defaults for everything else: n_fft 2048, hop_length 512, center = True, 128 Slaney mel filters over
    // 0 .. sr / 2, power_to_db(ref = 1, top_db = 80) over the clip, the orthonormal DCT
    dsp_mfcc_default_config(c);
    c->sample_rate = sample_rate;
    c->n_fft = 2048;
    c->frame_length = 2048;
    c->hop_length = 512;
    c->n_mels = 128;
    c->n_mfcc = n_mfcc;
    c->window = DSP_WINDOW_HANN;
    c->mel_norm = DSP_MELNORM_LIBROSA;
    c->log_mode = DSP_LOG_GLOBAL_REF1;
    c->spectrum = DSP_SPECTRUM_POWER;
    c->framing = DSP_FRAMING_CENTER;
    c->win_length = 0;
    c->prefilter = DSP_PREFILTER_NONE;
    c->fmin = 0.0f;
    c->fmax = 0.5f * (float)sample_rate;
    c->amin = 1e-10f;
    c->top_db = 80.0f;
}

int dsp_mfcc_frames_for(const dsp_mfcc_config *cfg, int num_samples, int max_frames)
{
    if (!cfg || max_frames <= 0) return 0;
    if (cfg->framing == DSP_FRAMING_CENTER) {
        // librosa.util.frame over the clip padded by n_fft / 2 zeros at both ends: 1 + n / hop frames
        if (num_samples <= 0 || cfg->hop_length <= 0) return 0;
        return (int)std::min<long>(1L + num_samples / cfg->hop_length, max_frames);
    }
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
    if (!cfg) return capi_fail(DSP_EINVAL, "cfg is NULL");
    {   // (the sanitizer tier's sweep found this entry point building tables for configurations dsp_mfcc_plan_create refuses --
        // sample_rate 0, fmin > fmax, n_fft 333: NaN tables rather than an error)
        std::string why;
        if (!valid_cfg(*cfg, why)) return capi_fail(DSP_EINVAL, why);
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
    if (prefilter != DSP_PREFILTER_BUTTER_1000_3000 && prefilter != DSP_PREFILTER_BUTTER_3000_7500) return capi_fail(DSP_EINVAL, "prefilter must name one of the two literal band-passes");
    double b[9], a[9];
    dsp_butter_bandpass(prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 1000 : 3000, prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 3000 : 7500, b, a);
    dsp::PrefilterScan sc;
    std::string why;
    if (!dsp::build_prefilter_scan(b, a, sc, why)) return capi_fail(DSP_EINVAL, why);
    if (steps4) for (int k = 0; k < 4; ++k) steps4[k] = sc.c_steps[k];
    return (sc.c_ok ? 1 : 0) | (sc.c_row_ok ? 2 : 0);
}

int dsp_mfcc_lane_tables(const dsp_mfcc_config *cfg, void *out, int size)
{
    if (!cfg) return capi_fail(DSP_EINVAL, "cfg is NULL");
    if (cfg->n_fft == 400) return capi_fail(DSP_EINVAL, "dsp_mfcc_lane_tables holds the 512-point kernel's tables: n_fft 400 has dsp_mfcc400_tables");
    if (!out) return (int)sizeof(dsp::LaneTables512);
    if (size != (int)sizeof(dsp::LaneTables512)) return capi_fail(DSP_EINVAL, "size != sizeof(LaneTables512)");
    std::string why;
    auto t = std::make_unique<dsp::LaneTables512>();
    if (!valid_cfg(*cfg, why) || !dsp::build_lane_tables_512(*cfg, *t, why)) return capi_fail(DSP_EINVAL, why);
    std::memcpy(out, t.get(), sizeof(*t));
    return DSP_OK;
}

int dsp_mfcc400_tables(const dsp_mfcc_config *cfg, void *out, int size)
{
    if (!cfg) return capi_fail(DSP_EINVAL, "cfg is NULL");
    if (!out) return (int)sizeof(dsp::Tables400);
    if (size != (int)sizeof(dsp::Tables400)) return capi_fail(DSP_EINVAL, "size != sizeof(Tables400)");
    std::string why;
    auto t = std::make_unique<dsp::Tables400>();
    if (!valid_cfg(*cfg, why) || !dsp::build_tables_400(*cfg, *t, why)) return capi_fail(DSP_EINVAL, why);
    std::memcpy(out, t.get(), sizeof(*t));
    return DSP_OK;
}

int dsp_mfcc1024_tables(const dsp_mfcc_config *cfg, void *out, int size)
{
    if (!cfg) return capi_fail(DSP_EINVAL, "cfg is NULL");
    if (!out) return (int)sizeof(dsp::GenTables1024);
    if (size != (int)sizeof(dsp::GenTables1024)) return capi_fail(DSP_EINVAL, "size != sizeof(GenTables1024)");
    std::string why;
    auto t = std::make_unique<dsp::GenTables1024>();
    if (!valid_cfg(*cfg, why) || !dsp::build_gen_tables_1024(*cfg, *t, why)) return capi_fail(DSP_EINVAL, why);
    std::memcpy(out, t.get(), sizeof(*t));
    return DSP_OK;
}

int dsp_mfcc2048_tables(const dsp_mfcc_config *cfg, void *out, int size)
{
    if (!cfg) return capi_fail(DSP_EINVAL, "cfg is NULL");
    if (!out) return (int)sizeof(dsp::GenTables2048);
    if (size != (int)sizeof(dsp::GenTables2048)) return capi_fail(DSP_EINVAL, "size != sizeof(GenTables2048)");
    std::string why;
    auto t = std::make_unique<dsp::GenTables2048>();
    if (!valid_cfg(*cfg, why) || !dsp::build_gen_tables_2048(*cfg, *t, why)) return capi_fail(DSP_EINVAL, why);
    std::memcpy(out, t.get(), sizeof(*t));
    return DSP_OK;
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
    else { capi_fail(DSP_EINVAL, "invalid bandpass range"); return 0; }   // classifier.c:402-407
    std::memcpy(b, sb, sizeof(B1));
    std::memcpy(a, sa, sizeof(A1));
    return 1;
}

// What `kernel` (a DSP_KERNEL_* id the plan's n_fft has) means on this plan: the family, its chunk granule and the occupancy of the
// forms its entries launch.  The plan's device is current.
static dsp::PlanKernel resolve_kernel(const dsp_mfcc_plan *p, int kernel)
{
    using K = dsp::PlanKernel;
    const dsp_mfcc_config &c = p->cfg;
    K k;
    if (c.n_fft == 400) {
        k.family = K::FFT400;
        k.per_cu = dsp::mfcc400_blocks_per_cu(c.n_mels);
    } else if (c.n_fft == 2048) {
        const bool aub = c.spectrum != DSP_SPECTRUM_POWER || c.log_mode == DSP_LOG_LOG10_FLOOR || c.framing == DSP_FRAMING_STREAM;
        k.family = aub ? K::FFT2048_AUBIO : K::FFT2048;
        k.per_cu = dsp::mfcc2048_blocks_per_cu(c.n_mels, false, aub);
        k.per_cu_fused = dsp::mfcc2048_blocks_per_cu(c.n_mels, true, aub);
    } else if (c.n_fft == 1024) {
        const bool wave = p->wave1024_fits && kernel != DSP_KERNEL_ROW, full = c.frame_length == 1024;
        k.family = wave ? K::FFT1024_WAVE : K::FFT1024_ROW;
        k.granule = wave ? 8 : 1;
        k.per_cu = wave ? dsp::mfcc1024_wave_blocks_per_cu(full) : dsp::mfcc1024_blocks_per_cu(full);
        if (wave && p->d_scan) k.per_cu_prefilter = dsp::mfcc1024_wave_blocks_per_cu(true, true);
    } else {
        const bool tile = kernel == DSP_KERNEL_WAVE && c.log_mode == DSP_LOG_PER_FRAME_MAX;
        k.family = tile ? K::FFT512_TILE : K::FFT512_FRAME;
        k.granule = tile ? 8 : 1;
        k.per_cu = dsp::mfcc512_blocks_per_cu(p->host.dct_split, p->host.dct_len, p->host.mel_gather, c.frame_length == 512, tile);
        if (tile) k.per_cu_fused = k.per_cu;
    }
    return k;
}

// n_fft 400 plans (dsp_mfcc_speaker_config) run float frames, clips and ragged batches on their own kernel and nothing else: `what` names
// the entry that refuses one
static int refuse_400(const char *what)
{
    return capi_fail(DSP_EINVAL, std::string(what) + " is not implemented for n_fft 400 plans (float frames, clips and ragged batches only)");
}

int dsp_mfcc_plan_create(const dsp_mfcc_config *cfg, int device, dsp_mfcc_plan **out)
{
    if (!cfg || !out) return capi_fail(DSP_EINVAL, "cfg/out is NULL");
    *out = nullptr;
    std::string why;
    if (!valid_cfg(*cfg, why)) return capi_fail(DSP_EINVAL, why);
    auto lane = std::make_unique<dsp::LaneTables512>();      // (zeros for the other transform lengths, as the plan's own always were)
    std::unique_ptr<dsp::GenTables1024> gen;
    std::unique_ptr<dsp::GenTables2048> g2k;
    std::unique_ptr<dsp::Tables400> t400;
    if (cfg->n_fft == 400) {
        t400 = std::make_unique<dsp::Tables400>();
        if (!dsp::build_tables_400(*cfg, *t400, why)) return capi_fail(DSP_EINVAL, why);
    } else if (cfg->n_fft == 2048) {
        g2k = std::make_unique<dsp::GenTables2048>();
        if (!dsp::build_gen_tables_2048(*cfg, *g2k, why)) return capi_fail(DSP_EINVAL, why);
    } else if (cfg->n_fft == 1024) {
        gen = std::make_unique<dsp::GenTables1024>();
        if (!dsp::build_gen_tables_1024(*cfg, *gen, why)) return capi_fail(DSP_EINVAL, why);
    } else if (cfg->n_fft != 512) return capi_fail(DSP_EINVAL, "internal: no tables for this n_fft");
    else if (!dsp::build_lane_tables_512(*cfg, *lane, why)) return capi_fail(DSP_EINVAL, why);
    if (const int rc = dsp::check_device(device)) return rc;
    return dsp::create_on_device(device, out, [&](dsp_mfcc_plan &plan) -> int {
        dsp_mfcc_plan *const p = &plan;
        p->cfg = *cfg;
        p->host = *lane;
        hipDeviceProp_t prop;
        hipError_t e = hipGetDeviceProperties(&prop, device);
        if (e == hipSuccess) e = dsp::upload(p->d_tables, p->host);
        if (e == hipSuccess && gen) e = dsp::upload(p->d_gen_tables, *gen);
        if (e == hipSuccess && g2k) e = dsp::upload(p->d_tables2048, *g2k);
        if (e == hipSuccess && t400) e = dsp::upload(p->d_tables400, *t400);
        p->wave1024_fits = gen && gen->n_chunk_slots <= 3;
        if (e == hipSuccess && cfg->prefilter != DSP_PREFILTER_NONE && cfg->frame_length == 1024 && p->wave1024_fits) {
            // BASELINE config 3 in ONE pass: the per-frame Butterworth as a scan inside the MFCC kernel (tables.hpp PrefilterScan)
            double b[9], a[9];
            dsp_butter_bandpass(cfg->prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 1000 : 3000,
                                cfg->prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 3000 : 7500, b, a);
            dsp::PrefilterScan sc;
            if (!dsp::build_prefilter_scan(b, a, sc, why)) return capi_fail(DSP_EINVAL, why);
            if (sc.c_ok && sc.c_row_ok) {      // the kernel runs the cascade form (its scan in row form); coefficients without it (none of the two literal sets) take the two-pass path
                e = dsp::upload(p->d_scan, sc);
                for (int k = 0; k < 4; ++k) p->scan_steps[k] = sc.c_steps[k];
            }
        }
        if (e != hipSuccess) return capi_fail(DSP_EHIP, std::string("plan_create: ") + hipGetErrorString(e));
        p->n_cu = prop.multiProcessorCount;
        p->run = resolve_kernel(p, DSP_KERNEL_WAVE);
        if (const char *k = std::getenv("DSP_AMD_KERNEL")) {
            // an A/B switch, not a requirement: a value this plan's n_fft has no kernel for is reported and ignored -- an
            // environment left over from the removed 512-point experiments must not make every plan_create fail
            if (dsp_mfcc_plan_set_kernel(p, std::atoi(k)) != DSP_OK)
                std::fprintf(stderr, "libdsp_amd: DSP_AMD_KERNEL=%s ignored (%s); using the default kernel\n", k, dsp_last_error());
        }
        return DSP_OK;
    });
}

void dsp_mfcc_plan_destroy(dsp_mfcc_plan *p) { dsp::destroy(p); }

int dsp_mfcc_plan_config(const dsp_mfcc_plan *p, dsp_mfcc_config *cfg)
{
    if (!p || !cfg) return capi_fail(DSP_EINVAL, "plan/cfg is NULL");
    *cfg = p->cfg;
    return DSP_OK;
}

int dsp_mfcc_plan_set_kernel(dsp_mfcc_plan *p, int kernel)
{
    if (!p || (kernel != DSP_KERNEL_WAVE && kernel != DSP_KERNEL_ROW && kernel != DSP_KERNEL_WAVE_FRAME && kernel != DSP_KERNEL_PAIR)) return capi_fail(DSP_EINVAL, "bad kernel id");
    // DSP_KERNEL_ROW on a 1024-point plan selects the general Stockham kernel (a product path: the fallback for filterbanks
    // the wave kernel's tables do not hold); the 512-point row / pair kernels were measured dead ends (0.537 ms and 0.44-0.45 ms
    // against 0.41 ms for the default kernel, profiles/r02_wave_priority_ab.txt) and have been removed
    if (kernel != DSP_KERNEL_WAVE && p->cfg.n_fft == 400) return refuse_400("dsp_mfcc_plan_set_kernel with anything but DSP_KERNEL_WAVE");
    if (kernel == DSP_KERNEL_PAIR || (kernel == DSP_KERNEL_ROW && p->cfg.n_fft != 1024))
        return capi_fail(DSP_EINVAL, "DSP_KERNEL_ROW / DSP_KERNEL_PAIR: the 512-point row and pair kernels were removed (measured slower than the default kernel)");
    dsp::DeviceScope dsp_device_scope_(p->device);      // the occupancy queries
    p->kernel = kernel;
    p->run = resolve_kernel(p, kernel);
    return DSP_OK;
}

int dsp_mfcc_plan_set_launch(dsp_mfcc_plan *p, int blocks_per_cu, int frames_per_chunk)
{
    if (!p || blocks_per_cu < 0 || frames_per_chunk < 0) return capi_fail(DSP_EINVAL, "bad launch knobs");
    p->blocks_per_cu = blocks_per_cu;
    p->chunk = frames_per_chunk;
    return DSP_OK;
}

}  // extern "C"

// ragged: the spans (caller's order, clips of >= 1 frame, ClipSpan::frame0 = first output row) and behind them the chunk table of the
// kernels' RaggedCursor (built on the device for `chunk`), in the leased ring slot
static int ragged_mfcc_spans(dsp_mfcc_plan *p, const RaggedBatch &rg, long n_frames, int chunk, dsp::SpanRing::Lease &slot, hipStream_t st)
{
    const size_t span_bytes = (size_t)rg.n_spans * sizeof(dsp::ClipSpan);
    const long n_chunks = (n_frames + chunk - 1) / chunk;
    DSP_CAPI_HIP(p->spans.acquire(span_bytes + (size_t)n_chunks * sizeof(int), slot));
    auto *h = static_cast<dsp::ClipSpan *>(slot.h());
    long j = 0;
    for (long c = 0; c < rg.n_clips; ++c) {
        const int frames = (int)(rg.frame_offsets[c + 1] - rg.frame_offsets[c]);
        const long n = rg.lengths ? rg.lengths[c] : rg.offsets[c + 1] - rg.offsets[c];
        if (frames > 0) h[j++] = dsp::ClipSpan{rg.offsets[c], (int)n, frames, c, rg.frame_offsets[c]};
    }
    DSP_CAPI_HIP(slot.upload(span_bytes, st));
    DSP_CAPI_HIP(dsp::launch_ragged_chunk_map(static_cast<const dsp::ClipSpan *>(slot.d()), rg.n_spans, chunk,
                                         reinterpret_cast<int *>(static_cast<char *>(slot.d()) + span_bytes), st));
    return DSP_OK;
}

// DSP_LOG_GLOBAL_REF1 over clips (clip-global top_db): pass 1 writes each frame's maximum, a tiny kernel turns them into one floor per
// clip, pass 2 is the normal kernel clipping at that floor.  launch(args) enqueues the plan's MFCC kernel.
template <class Launch> static int two_pass_floor(dsp_mfcc_plan *p, dsp::Mfcc512Args &a, hipStream_t st, const Launch &launch)
{
    const long n_clips = a.spans ? a.n_clips : a.n_frames / a.frames_per_clip;
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_CAPI_HIP(p->d_frame_max.reserve((size_t)a.n_frames * sizeof(float)));
    DSP_CAPI_HIP(p->d_clip_floor.reserve((size_t)n_clips * sizeof(float)));
    a.frame_max = p->d_frame_max;
    DSP_CAPI_HIP(launch(a));
    if (a.spans) DSP_CAPI_HIP(dsp::launch_clip_floor_ragged(p->d_frame_max, a.spans, n_clips, a.top_db, p->d_clip_floor, st));
    else DSP_CAPI_HIP(dsp::launch_clip_floor(p->d_frame_max, n_clips, a.frames_per_clip, a.top_db, p->d_clip_floor, st));
    a.frame_max = nullptr;
    a.clip_floor = p->d_clip_floor;
    DSP_CAPI_HIP(launch(a));
    return DSP_OK;
}

int dsp::plan_accepts(const dsp_mfcc_plan *p, PlanUse use, int in_kind)
{
    using K = dsp::PlanKernel;
    const dsp_mfcc_config &c = p->cfg;
    const K::Family fam = p->run.family;
    const bool aub = fam == K::FFT2048_AUBIO, wave = p->kernel == DSP_KERNEL_WAVE, prefilter = c.prefilter != DSP_PREFILTER_NONE;
    // a 512-point plan's shape against the kernel's forms (the fused kernels and int16 rows are forms of the tile epilogue)
    const auto form = [&](Mfcc512Use u) {
        return fam == K::FFT512_TILE && mfcc512_has_form(u, p->host.dct_split, p->host.dct_len, p->host.mel_gather, c.frame_length, in_kind, true);
    };
    // centred 2048-point plans (dsp_mfcc_librosa_config) run float frames, clips and ragged batches, as the 400-point plans do
    if (c.framing == DSP_FRAMING_CENTER && fam != K::FFT400 && (in_kind != 0 || (use != PlanUse::Frames && use != PlanUse::Clips && use != PlanUse::Ragged)))
        return capi_fail(DSP_EINVAL, "framing: DSP_FRAMING_CENTER plans at n_fft 2048 take float frames, clips and ragged batches only (no PCM16 ingestion, "
                                     "fused clip kernel, scanner or stream session)");
    switch (use) {
    case PlanUse::FusedLabel:
        if (fam == K::FFT400) return refuse_400("the fused clip -> label path");
        if ((c.n_fft != 512 && c.n_fft != 2048) || (c.log_mode != DSP_LOG_PER_FRAME_MAX && c.log_mode != DSP_LOG_LOG10_FLOOR) || prefilter || !wave)
            return capi_fail(DSP_EINVAL, "the fused clip -> label path runs on the 512- and 2048-point wave-per-frame kernels, per-frame log modes");
        if (in_kind != 0 && !aub && !form(Mfcc512Use::Label))
            return capi_fail(DSP_EINVAL, "int16 input of the fused clip -> label kernel: the reference framing (n_fft 512, frame 400, 40 mel filters, up to 20 coefficients) "
                                    "or the scrubjay_infer.c front end (dsp_mfcc_scrubjay_infer_config)");
        return DSP_OK;
    case PlanUse::FusedStop:
        if (fam == K::FFT400) return refuse_400("classify_signal (the fused clip -> probability kernel and its two-kernel form)");
        return !prefilter && form(Mfcc512Use::Stop) ? 1 : 0;
    case PlanUse::ScrubjayScan:
        // the plans whose rows do not depend on the window, on the fused clip -> label kernel's front ends (what per-window equality is against)
        if (fam == K::FFT400) return refuse_400("a scrub-jay scan");
        if (c.log_mode == DSP_LOG_GLOBAL_REF1) return capi_fail(DSP_EINVAL, "DSP_LOG_GLOBAL_REF1 plans cannot be scanned: the top_db floor spans the window");
        if (prefilter || c.n_fft == 1024) return capi_fail(DSP_EINVAL, "scans run on the ragged MFCC matrix: prefilter plans and n_fft 1024 are not supported");
        if (!wave) return capi_fail(DSP_EINVAL, "scans run on the wave-per-frame kernel (DSP_KERNEL_WAVE), as the fused clip -> label path");
        if (in_kind != 0 && !aub && !form(Mfcc512Use::Clips))
            return capi_fail(DSP_EINVAL, "int16 input of the scrub-jay scan: the ragged MFCC matrix takes it on the scrubjay_infer.c front end "
                                         "(dsp_mfcc_scrubjay_infer_config) and on the 512-point framing with up to 13 coefficients of 40 mel filters");
        return DSP_OK;
    case PlanUse::Scan:
        if (fam == K::FFT400) return refuse_400("a scanner or stream session");
        if (c.n_fft != 512 || c.log_mode != DSP_LOG_PER_FRAME_MAX || c.framing != DSP_FRAMING_COMPLETE || prefilter)
            return capi_fail(DSP_EINVAL, "scans need a plan whose rows do not depend on the window: n_fft 512, DSP_LOG_PER_FRAME_MAX, DSP_FRAMING_COMPLETE, "
                                         "no prefilter");
        break;
    case PlanUse::Clips:
        if (prefilter)
            return capi_fail(DSP_EINVAL, in_kind == 0 ? "the per-frame prefilter applies to independent frames only"
                                                      : "the per-frame prefilter applies to independent float frames only");
        break;
    case PlanUse::Ragged:
        if (prefilter) return capi_fail(DSP_EINVAL, "ragged MFCC matrices: prefilter plans are not supported (the per-frame prefilter applies to independent frames)");
        if (c.n_fft == 1024) return capi_fail(DSP_EINVAL, "ragged MFCC matrices run on the 400-, 512- and 2048-point kernels: n_fft 1024 is not supported");
        break;
    case PlanUse::Frames: break;
    }
    // MFCC rows: every family takes float samples; int16 is converted in the load of the forms that have one
    if (in_kind == 0) return DSP_OK;
    if (fam == K::FFT400) return refuse_400("PCM16 ingestion");
    if (aub && use != PlanUse::Frames) return DSP_OK;
    if (fam != K::FFT512_TILE)
        return capi_fail(DSP_EINVAL, "PCM16 ingestion runs on the 512-point wave-per-frame kernel (per-frame log mode) and on the 2048-point scrubjay_infer.c front end");
    if (!form(use == PlanUse::Frames ? Mfcc512Use::Frames : Mfcc512Use::Clips))
        return capi_fail(DSP_EINVAL, std::string("PCM16 ingestion on a 512-point plan: of the kernel's shapes, MFCC rows take int16 clips and ragged batches for ") +
                                         dsp::kMfcc512RowsPcm16Shapes);
    return DSP_OK;
}

int dsp::mfcc_run(dsp_mfcc_plan *p, const MfccJob &job)
{
    const long n_frames = job.n_frames;
    const int frames_per_clip = job.frames_per_clip, in_kind = job.in_kind;
    const RaggedBatch *rg = job.ragged;
    if (n_frames == 0) return DSP_OK;
    DSP_ON_DEVICE(p->device);       // the caller's current device may be another GPU: tables and workspaces live on the plan's
    hipStream_t st = (hipStream_t)job.stream;
    const bool clip_mode = frames_per_clip > 0 || rg;
    const bool single_clip = frames_per_clip > 0 && n_frames == frames_per_clip;   // stride unused
    if (const int rc = dsp::check_aligned(job.in, in_kind, !single_clip, job.clip_stride)) return rc;
    dsp::Mfcc512Args a = dsp::plan_args(p, job.in, in_kind, clip_mode);
    a.out = job.out;
    a.n_frames = n_frames;
    a.clip_stride = job.clip_stride;
    a.frames_per_clip = frames_per_clip;
    a.samples_per_clip = job.samples_per_clip;
    using K = dsp::PlanKernel;
    const K &k = p->run;
    if (a.center_framing && job.samples_per_clip <= 0 && !rg) return capi_fail(DSP_EINVAL, "internal: centred framing without the clip length");
    if (a.stream_framing && job.samples_per_clip <= 0 && !rg) return capi_fail(DSP_EINVAL, "internal: stream framing without the clip length");
    if (job.fused_prefilter && !(k.family == K::FFT1024_WAVE && p->d_scan)) return capi_fail(DSP_EINVAL, "internal: fused prefilter without its tables");
    a.chunk = p->chunk > 0 ? p->chunk : 8;
    a.chunk = ((a.chunk + k.granule - 1) / k.granule) * k.granule;   // whole items (tile: half-tiles of 8 frames) per chunk
    dsp::SpanRing::Lease slot;
    if (rg) {
        const int rc = ragged_mfcc_spans(p, *rg, n_frames, a.chunk, slot, st);
        if (rc < 0) return rc;
        a.spans = static_cast<const dsp::ClipSpan *>(slot.d());
        a.n_clips = rg->n_spans;
    }
    const int blocks = dsp::grid(p, job.fused_prefilter ? k.per_cu_prefilter : k.per_cu, (n_frames + a.chunk - 1) / a.chunk);
    auto launch = [&](const dsp::Mfcc512Args &x) {
        switch (k.family) {
        case K::FFT400: return dsp::launch_mfcc400(x, p->d_tables400, blocks, st);
        case K::FFT2048: case K::FFT2048_AUBIO: return dsp::launch_mfcc2048(x, p->d_tables2048, blocks, st, false);
        case K::FFT1024_WAVE: return dsp::launch_mfcc1024_wave(x, p->d_gen_tables, blocks, st, job.fused_prefilter ? p->d_scan : nullptr, p->scan_steps);
        case K::FFT1024_ROW: return dsp::launch_mfcc1024(x, p->d_gen_tables, blocks, st);
        case K::FFT512_TILE: case K::FFT512_FRAME: break;
        }
        return dsp::launch_mfcc512(x, p->host.dct_split, p->host.dct_len, p->host.mel_gather, blocks, st, k.family == K::FFT512_TILE);
    };
    if (a.log_mode == DSP_LOG_GLOBAL_REF1 && clip_mode) return two_pass_floor(p, a, st, launch);
    DSP_CAPI_HIP(launch(a));      // (DSP_LOG_GLOBAL_REF1 on independent frames: one pass, every frame its own clip)
    return DSP_OK;
}

// The argument checks of equal clips, device and host form alike, in the order a bad call is refused: the frames per clip, 0 where
// there is nothing to do (no clip, or clips too short for a frame), or < 0.  ask_plan: false leaves plan_accepts(PlanUse::Clips) out
// (kFloatHostClipsAskPlan below is its only user)
static int check_clips(dsp_mfcc_plan *p, const void *in, int in_kind, long n_clips, int samples_per_clip, long clip_stride, const float *out, int max_frames,
                       bool ask_plan = true)
{
    if (in_kind < 0) return in_kind;
    if (!p || n_clips < 0) return capi_fail(DSP_EINVAL, "bad argument");
    if (ask_plan)
        if (const int rc = plan_accepts(p, dsp::PlanUse::Clips, in_kind)) return rc;
    const int t = dsp_mfcc_frames_for(&p->cfg, samples_per_clip, max_frames);
    if (t == 0 || n_clips == 0) return 0;
    if (!in || !out) return capi_fail(DSP_EINVAL, "NULL buffer");
    if (n_clips > 1 && clip_stride < samples_per_clip) return capi_fail(DSP_EINVAL, "clip_stride < samples_per_clip");
    return t;
}

int dsp::mfcc_clips(dsp_mfcc_plan *p, const void *d_in, int in_kind, long n_clips, int samples_per_clip, long clip_stride, float *d_out, int max_frames,
                    void *stream)
{
    const int t = check_clips(p, d_in, in_kind, n_clips, samples_per_clip, clip_stride, d_out, max_frames);
    if (t <= 0) return t;
    const int rc = mfcc_run(p, {.in = d_in, .in_kind = in_kind, .out = d_out, .n_frames = n_clips * (long)t, .frames_per_clip = t,
                               .samples_per_clip = samples_per_clip, .clip_stride = clip_stride, .stream = stream});
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
        const long n = lengths ? (offsets[c] >= 0 && lengths[c] >= 0 && lengths[c] <= INT32_MAX ? lengths[c] : capi_fail(DSP_EINVAL, "internal: bad span"))
                               : dsp::ragged_clip_length(offsets, c);
        if (n < 0) return n;
        const int t = dsp_mfcc_frames_for(&cfg, (int)n, max_frames);
        frame_offsets[c + 1] = frame_offsets[c] + t;
        tm = std::max(tm, t);
    }
    if (t_max) *t_max = tm;
    return frame_offsets[n_clips];
}

// The argument checks of a ragged batch, device and host form alike, in the order a bad call is refused: the batch's frame offsets
// (ragged_frame_offsets), their total -- returned; 0: nothing to do; or < 0 --, the longest clip's frames, the clips that have any
struct RaggedFrames { std::vector<long> fo; long total = 0, n_spans = 0; int t_max = 0; };
static long check_clips_ragged(dsp_mfcc_plan *p, const void *in, int in_kind, long n_clips, const long *offsets, int max_frames, const float *out,
                               const long *lengths, RaggedFrames &r)
{
    if (in_kind < 0) return in_kind;
    if (!p || n_clips < 0 || !offsets) return capi_fail(DSP_EINVAL, "bad argument");
    if (const int rc = plan_accepts(p, dsp::PlanUse::Ragged, in_kind)) return rc;
    if (n_clips >= (1L << 31)) return capi_fail(DSP_EINVAL, "too many clips");
    r.fo.resize((size_t)n_clips + 1);
    r.total = ragged_frame_offsets(p->cfg, offsets, n_clips, max_frames, r.fo.data(), &r.t_max, lengths);
    if (r.total <= 0) return r.total;
    if (!in || !out) return capi_fail(DSP_EINVAL, "NULL buffer");
    for (long c = 0; c < n_clips; ++c) r.n_spans += r.fo[(size_t)c + 1] > r.fo[(size_t)c];
    return r.total;
}

int dsp::mfcc_clips_ragged(dsp_mfcc_plan *p, const void *d_in, int in_kind, long n_clips, const long *offsets, int max_frames, float *d_out,
                           void *stream, const long *lengths)
{
    RaggedFrames r;
    if (const long total = check_clips_ragged(p, d_in, in_kind, n_clips, offsets, max_frames, d_out, lengths, r); total <= 0) return (int)total;
    RaggedBatch rg{offsets, r.fo.data(), n_clips, r.n_spans, lengths};
    const int rc = mfcc_run(p, {.in = d_in, .in_kind = in_kind, .out = d_out, .n_frames = r.total, .ragged = &rg, .stream = stream});
    return rc < 0 ? rc : r.t_max;
}

extern "C" {

int dsp_mfcc_frames_device(dsp_mfcc_plan *p, const float *d_frames, long n_frames, float *d_out, void *stream)
{
    if (!p || n_frames < 0 || (n_frames > 0 && (!d_frames || !d_out))) return capi_fail(DSP_EINVAL, "bad argument");
    MfccJob job{.in = d_frames, .out = d_out, .n_frames = n_frames, .stream = stream};
    if (p->cfg.prefilter == DSP_PREFILTER_NONE) return mfcc_run(p, job);
    // BASELINE config 3: 8th-order Butterworth (donut-classifier/classifier.c:420-446, float64) over each
    // frame from zero state, rounded to float, then the MFCC chain.
    // One pass (1024-sample frames on the wave kernel, 16-byte aligned input): the filter runs inside the MFCC kernel as a
    // float64 parallel-form scan over the wave's lanes -- the frame is read once, nothing filtered is written.  This entry
    // point is tolerance-gated (1e-4 of the frame's L-inf norm); the scan equals the serial recurrence to ~1e-13 before the
    // rounding to float.  dsp_butter_bandpass_filter_* keep the bit-exact serial recurrence.
    if (p->run.per_cu_prefilter > 0 && (reinterpret_cast<uintptr_t>(d_frames) & 15) == 0 && !std::getenv("DSP_AMD_PREFILTER_TWO_PASS")) {
        job.fused_prefilter = true;
        return mfcc_run(p, job);
    }
    // Otherwise two passes: filtered frames go through a bounded workspace (sub-batches of <= 1 Mi frames).
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_ON_DEVICE(p->device);
    const int fl = p->cfg.frame_length;
    const long sub = std::min<long>(n_frames, 1L << 20);
    DSP_CAPI_HIP(p->d_filtered.reserve((size_t)sub * fl * sizeof(float)));
    dsp::IirCoefD c;
    dsp_butter_bandpass(p->cfg.prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 1000 : 3000,
                        p->cfg.prefilter == DSP_PREFILTER_BUTTER_1000_3000 ? 3000 : 7500, c.b, c.a);
    for (long f0 = 0; f0 < n_frames; f0 += sub) {
        const long cnt = std::min(sub, n_frames - f0);
        DSP_CAPI_HIP(dsp::launch_iir_f64_on_f32(d_frames + f0 * fl, cnt, fl, fl, c, p->d_filtered, (hipStream_t)stream));
        const int rc = mfcc_run(p, {.in = p->d_filtered, .out = d_out + f0 * p->cfg.n_mfcc, .n_frames = cnt, .stream = stream});
        if (rc < 0) return rc;
    }
    return DSP_OK;
}

int dsp_mfcc_clips_device(dsp_mfcc_plan *p, const float *d_signal, long n_clips, int samples_per_clip,
                          long clip_stride, float *d_out, int max_frames, void *stream)
{
    return dsp::mfcc_clips(p, d_signal, 0, n_clips, samples_per_clip, clip_stride, d_out, max_frames, stream);
}

int dsp_mfcc_clips_pcm16_device(dsp_mfcc_plan *p, const int16_t *d_pcm, long n_clips, int samples_per_clip,
                                long clip_stride, int channels, int stereo_mode, float *d_out, int max_frames, void *stream)
{
    return dsp::mfcc_clips(p, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, samples_per_clip, clip_stride, d_out, max_frames, stream);
}

long dsp_mfcc_ragged_frame_offsets(const dsp_mfcc_config *cfg, const long *offsets, long n_clips, int max_frames, long *frame_offsets)
{
    if (!cfg || !offsets || !frame_offsets || n_clips < 0) return capi_fail(DSP_EINVAL, "bad argument (cfg, offsets, frame_offsets non-NULL, n_clips >= 0)");
    std::string why;
    if (!valid_cfg(*cfg, why)) return capi_fail(DSP_EINVAL, why);
    return ragged_frame_offsets(*cfg, offsets, n_clips, max_frames, frame_offsets, nullptr);
}

int dsp_mfcc_clips_ragged_device(dsp_mfcc_plan *p, const float *d_signal, long n_clips, const long *offsets, int max_frames, float *d_out, void *stream)
{
    return dsp::mfcc_clips_ragged(p, d_signal, 0, n_clips, offsets, max_frames, d_out, stream);
}

int dsp_mfcc_clips_ragged_pcm16_device(dsp_mfcc_plan *p, const int16_t *d_pcm, long n_clips, const long *offsets, int channels, int stereo_mode,
                                       int max_frames, float *d_out, void *stream)
{
    return dsp::mfcc_clips_ragged(p, d_pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, max_frames, d_out, stream);
}

// ---- host batches: through the device's host pipeline (host_pipe.hpp), a chunk at a time ----

}  // extern "C"

namespace {

namespace host = dsp::host;
// uniform items of a plan (frames, or clips of one length) from `in`, an item's results being out_item floats.
// run(d_in, count, d_out, stream) enqueues the kernels of a chunk of `count` items.
template <class Run> int host_uniform(dsp_mfcc_plan *p, const void *in, host::UniformLayout l, float *out, size_t out_item, const Run &run)
{
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_ON_DEVICE(p->device);
    host::Session hs;
    if (const int rc = hs.open(p->device, in, l)) return rc;
    return hs.run(in, l, host::Outs{{out}, {out_item * sizeof(float)}}, [&](long k, const void *d_in, void *const *d_out, hipStream_t st) {
        return run(d_in, (long)l.rows(k), static_cast<float *>(d_out[0]), st);
    });
}

// Whether dsp_mfcc_clips_host asks plan_accepts(PlanUse::Clips).  It never has: the device entry and the int16 host entry refuse a
// prefilter plan, float clips from host memory run on it without the filter.  Kept as it behaves; it looks like an oversight.
constexpr bool kFloatHostClipsAskPlan = false;

// equal clips of in_kind, staged at an even stride so that every frame start keeps the kernels' alignment; the frames per clip, or < 0
int host_clips(dsp_mfcc_plan *p, const void *signal, int in_kind, long n_clips, int samples_per_clip, long clip_stride, float *out, int max_frames,
               bool ask_plan = true)
{
    const int t = check_clips(p, signal, in_kind, n_clips, samples_per_clip, clip_stride, out, max_frames, ask_plan);
    if (t <= 0) return t;
    const size_t bps = in_kind == 1 ? 2 : 4;                                  // bytes per sample, all channels
    const long dstride = samples_per_clip + (samples_per_clip & 1);
    if (n_clips == 1) clip_stride = samples_per_clip;
    const int rc = host_uniform(p, signal, {n_clips, (size_t)clip_stride * bps, (size_t)dstride * bps, (size_t)samples_per_clip * bps, true}, out,
                                (size_t)t * p->cfg.n_mfcc, [&](const void *d_in, long cnt, float *d_out, hipStream_t st) {
                                    return mfcc_run(p, {.in = d_in, .in_kind = in_kind, .out = d_out, .n_frames = cnt * (long)t, .frames_per_clip = t,
                                                        .samples_per_clip = samples_per_clip, .clip_stride = dstride, .stream = st});
                                });
    return rc < 0 ? rc : t;
}

// a ragged batch of in_kind: chunks of whole clips, each one ragged device pass over its own samples with the offsets rebased
int host_clips_ragged(dsp_mfcc_plan *p, const void *signal, int in_kind, long n_clips, const long *offsets, int max_frames, float *out)
{
    RaggedFrames r;
    if (const long total = check_clips_ragged(p, signal, in_kind, n_clips, offsets, max_frames, out, nullptr, r); total <= 0) return (int)total;
    host::RaggedLayout l{offsets, n_clips, (size_t)(in_kind == 1 ? 2 : 4)};
    std::lock_guard<std::recursive_mutex> lock(p->mu);
    DSP_ON_DEVICE(p->device);
    host::Session hs;
    if (const int rc = hs.open(p->device, signal, l)) return rc;
    int t_max = 0;
    std::vector<long> rebased;
    // a chunk's results are the rows of its clips: fo[first[k]] .. fo[first[k + 1]]
    const host::Outs outs{{out}, {(size_t)p->cfg.n_mfcc * sizeof(float)}, r.fo.data()};
    const int rc = hs.run(signal, l, outs, [&](long k, const void *d_in, void *const *d_out, hipStream_t st) {
        const long c0 = l.first[(size_t)k], c1 = l.first[(size_t)k + 1];
        if (r.fo[(size_t)c1] == r.fo[(size_t)c0]) return (int)DSP_OK;      // a chunk of clips without frames
        l.rebase(k, rebased);
        const int t = dsp::mfcc_clips_ragged(p, d_in, in_kind, c1 - c0, rebased.data(), max_frames, static_cast<float *>(d_out[0]), st);
        t_max = std::max(t_max, t);
        return std::min(t, 0);
    });
    return rc < 0 ? rc : t_max;
}

}  // namespace

extern "C" {

int dsp_mfcc_frames_host(dsp_mfcc_plan *p, const float *frames, long n_frames, float *out)
{
    if (!p || n_frames < 0 || (n_frames > 0 && (!frames || !out))) return capi_fail(DSP_EINVAL, "bad argument");
    if (n_frames == 0) return DSP_OK;
    if (p->cfg.prefilter != DSP_PREFILTER_NONE) return capi_fail(DSP_EINVAL, "prefiltered plans take device buffers (dsp_mfcc_frames_device)");
    const size_t fb = (size_t)p->cfg.frame_length * sizeof(float);
    return host_uniform(p, frames, {n_frames, fb, fb, fb, false}, out, (size_t)p->cfg.n_mfcc, [&](const void *d_in, long cnt, float *d_out, hipStream_t st) {
        return mfcc_run(p, {.in = d_in, .out = d_out, .n_frames = cnt, .stream = st});
    });
}

int dsp_mfcc_clips_host(dsp_mfcc_plan *p, const float *signal, long n_clips, int samples_per_clip,
                        long clip_stride, float *out, int max_frames)
{
    return host_clips(p, signal, 0, n_clips, samples_per_clip, clip_stride, out, max_frames, kFloatHostClipsAskPlan);
}

int dsp_mfcc_clips_pcm16_host(dsp_mfcc_plan *p, const int16_t *pcm, long n_clips, int samples_per_clip, long clip_stride, int channels, int stereo_mode,
                              float *out, int max_frames)
{
    if (!p) return capi_fail(DSP_EINVAL, "plan is NULL");
    return host_clips(p, pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, samples_per_clip, clip_stride, out, max_frames);
}

int dsp_mfcc_clips_ragged_host(dsp_mfcc_plan *p, const float *signal, long n_clips, const long *offsets, int max_frames, float *out)
{
    if (!p) return capi_fail(DSP_EINVAL, "plan is NULL");
    if (!offsets) return capi_fail(DSP_EINVAL, "offsets is NULL");
    return host_clips_ragged(p, signal, 0, n_clips, offsets, max_frames, out);
}

int dsp_mfcc_clips_ragged_pcm16_host(dsp_mfcc_plan *p, const int16_t *pcm, long n_clips, const long *offsets, int channels, int stereo_mode,
                                     int max_frames, float *out)
{
    if (!p) return capi_fail(DSP_EINVAL, "plan is NULL");
    if (!offsets) return capi_fail(DSP_EINVAL, "offsets is NULL");
    return host_clips_ragged(p, pcm, dsp::pcm16_kind(channels, stereo_mode), n_clips, offsets, max_frames, out);
}

#ifdef DSP_PF_STAMPS
__attribute__((visibility("default"))) int dsp_debug_pf_stamps(unsigned long long *out, int count)     // tools/pf_stamps.py
{
    DSP_CAPI_HIP(hipDeviceSynchronize());
    DSP_CAPI_HIP(dsp::read_pf_stamps(out, count));
    return DSP_OK;
}
#endif
#ifdef DSP_RC_STAMPS
__attribute__((visibility("default"))) int dsp_debug_rc_stamps(unsigned long long *out, int count)     // diagnostic builds only (tools/rc_stamps.py)
{
    DSP_CAPI_HIP(hipDeviceSynchronize());
    DSP_CAPI_HIP(dsp::read_rc_stamps(out, count));
    return DSP_OK;
}
__attribute__((visibility("default"))) int dsp_debug_bd_stamps(unsigned long long *out, int count)
{
    DSP_CAPI_HIP(hipDeviceSynchronize());
    DSP_CAPI_HIP(dsp::read_bd_stamps(out, count));
    return DSP_OK;
}
#endif

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
    if (!signal || !out_mfcc) { capi_fail(DSP_EINVAL, "NULL buffer"); return 0; }
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
