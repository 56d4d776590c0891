// capi_vad.cpp -- the C ABI of voice activity detection (include/dsp_amd.h dsp_vad_*, dsp_rows_*): argument checks, all
// of them before a device is touched and in the order the header states, the host-only geometry, workspace size and trim spans, the
// offsets that travel into the caller's workspace, and the launches of vad_kernels.hip.  The stage keeps nothing between calls: what
// lives on the device lies in the caller's workspace, so there is no handle.
#include <cmath>
#include <cstdint>
#include <vector>

#include "capi_util.hpp"
#include "vad_kernels.hpp"

using dsp::capi_fail;

static_assert(sizeof(dsp_vad_config) == 56, "dsp_vad_config is 56 bytes (dsp_amd/lib.py VadConfig)");
static_assert(sizeof(dsp_vad_clip) == 32, "dsp_vad_clip is 32 bytes (dsp_amd/lib.py VAD_CLIP_DTYPE)");
static_assert(sizeof(dsp_vad_geometry) == 20, "dsp_vad_geometry is 20 bytes (dsp_amd/lib.py VadGeometry)");

namespace {

constexpr long kMaxClips = 1L << 31;      // exclusive

int check_config(const dsp_vad_config *cfg, dsp::VadGeometry &geo)
{
    if (!cfg) return capi_fail(DSP_EINVAL, "dsp_vad_config is NULL");
    std::string why;
    if (!dsp::vad_geometry(cfg->frame_length, cfg->hop_length, cfg->framing, geo, why)) return capi_fail(DSP_EINVAL, "dsp_vad_config: " + why);
    if (cfg->reference != DSP_VAD_REF_ABSOLUTE && cfg->reference != DSP_VAD_REF_MAX && cfg->reference != DSP_VAD_REF_MEAN)
        return capi_fail(DSP_EINVAL, "dsp_vad_config: reference must be DSP_VAD_REF_ABSOLUTE, DSP_VAD_REF_MAX or DSP_VAD_REF_MEAN");
    if (!(cfg->threshold_ratio >= 0.0 && std::isfinite(cfg->threshold_ratio))) return capi_fail(DSP_EINVAL, "dsp_vad_config: threshold_ratio must be finite and >= 0");
    if (!(cfg->floor_power >= 0.0)) return capi_fail(DSP_EINVAL, "dsp_vad_config: floor_power must be >= 0");
    if (cfg->context_frames < 0 || cfg->context_frames > dsp::kVadMaxContext) return capi_fail(DSP_EINVAL, "dsp_vad_config: context_frames must be 0 .. 64");
    if (cfg->pad_frames < 0 || cfg->pad_frames > dsp::kVadMaxContext) return capi_fail(DSP_EINVAL, "dsp_vad_config: pad_frames must be 0 .. 64");
    if (!(cfg->proportion > 0.0 && cfg->proportion <= 1.0)) return capi_fail(DSP_EINVAL, "dsp_vad_config: proportion must lie in (0, 1]");
    return DSP_OK;
}

int check_call(int device, long n_clips)
{
    if (device < 0) return capi_fail(DSP_EINVAL, "device index out of range");
    if (n_clips < 0) return capi_fail(DSP_EINVAL, "n_clips < 0");
    if (n_clips >= kMaxClips) return capi_fail(DSP_EINVAL, "2^31 clips or more in one call");
    return DSP_OK;
}

// the clips' row counts against their lengths: DSP_EINVAL naming the first clip with more rows than its samples give
int check_rows(const dsp_vad_config *cfg, const long *offsets, const long *frame_offsets, long n_clips)
{
    dsp_mfcc_config mfcc{};
    mfcc.frame_length = cfg->frame_length;
    mfcc.hop_length = cfg->hop_length;
    mfcc.framing = cfg->framing;
    for (long c = 0; c < n_clips; ++c) {
        const long n = dsp::ragged_clip_length(offsets, c);
        if (n < 0) return (int)n;
        const long rows = frame_offsets[c + 1] - frame_offsets[c], most = dsp_mfcc_frames_for(&mfcc, (int)n, INT_MAX);
        if (rows > most)
            return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + " brings " + std::to_string(rows) + " rows, its " + std::to_string(n) + " samples give " +
                                             std::to_string(most));
    }
    return DSP_OK;
}

int check_workspace(const void *ws, long bytes, size_t need)
{
    if (!ws) return capi_fail(DSP_EINVAL, "d_workspace is NULL");
    if (reinterpret_cast<uintptr_t>(ws) & 255) return capi_fail(DSP_EINVAL, "d_workspace must be 256-byte aligned");
    if (bytes < 0 || (size_t)bytes < need)
        return capi_fail(DSP_EINVAL, "d_workspace holds " + std::to_string(bytes) + " bytes, the call needs " + std::to_string(need) + " (dsp_vad_workspace_bytes)");
    return DSP_OK;
}

// the offsets of one call from 0, as the kernels read them, and the tiles they give
struct Spans {
    std::vector<long> host;      // so | fo | to, n + 1 each (so absent: zeros)
    long n = 0, rows = 0, tiles = 0;
    void fill(const long *offsets, const long *frame_offsets, long n_clips)
    {
        n = n_clips;
        const size_t n1 = (size_t)n + 1;
        host.assign(3 * n1, 0);
        long *so = host.data(), *fo = so + n1, *to = fo + n1;
        for (long c = 0; c < n; ++c) {
            if (offsets) so[c + 1] = offsets[c + 1] - offsets[0];
            fo[c + 1] = frame_offsets[c + 1] - frame_offsets[0];
            to[c + 1] = to[c] + dsp::vad_tiles(fo[c + 1] - fo[c]);
        }
        rows = fo[n];
        tiles = to[n];
    }
    // into the workspace, on the stream, in one copy; the copy has left the host's array when this returns (pageable memory)
    hipError_t upload(const dsp::VadWorkspace &ws, hipStream_t st) const
    {
        return hipMemcpyAsync(ws.so, host.data(), host.size() * sizeof(long), hipMemcpyHostToDevice, st);
    }
};

dsp::VadDecision decision_of(const dsp_vad_config *cfg)
{
    return dsp::VadDecision{cfg->reference, cfg->threshold_ratio, cfg->floor_power, cfg->proportion, cfg->context_frames, cfg->pad_frames};
}

// ws.counts[n] -> kept_offsets[n + 1], the one wait for the stream
int download_kept_offsets(const dsp::VadWorkspace &ws, long n, long *kept_offsets, hipStream_t st)
{
    kept_offsets[0] = 0;
    DSP_CAPI_HIP(hipMemcpyAsync(kept_offsets + 1, ws.counts, (size_t)n * sizeof(long), hipMemcpyDeviceToHost, st));
    DSP_CAPI_HIP(hipStreamSynchronize(st));
    for (long c = 0; c < n; ++c) kept_offsets[c + 1] += kept_offsets[c];
    return DSP_OK;
}

enum class Call { Power, Decide, Run };      // d_power: written (Power), read (Decide), absent (Run: the power stays in the workspace)

int vad_call(Call call, int device, const dsp_vad_config *cfg, const float *d_signal, double *d_power, long n_clips, const long *offsets,
             const long *frame_offsets, uint8_t *d_flags, float *d_level_db, dsp_vad_clip *d_clips, long *kept_offsets, void *d_workspace,
             long workspace_bytes, void *stream)
{
    const bool from_signal = call != Call::Decide, decide = call != Call::Power, keeps_power = call == Call::Run;
    dsp::VadGeometry geo;
    if (const int rc = check_config(cfg, geo)) return rc;
    if (const int rc = check_call(device, n_clips)) return rc;
    if (decide && !kept_offsets) return capi_fail(DSP_EINVAL, "kept_offsets is NULL");
    if (n_clips == 0) {
        if (decide) kept_offsets[0] = 0;
        return DSP_OK;
    }
    if (from_signal && !offsets) return capi_fail(DSP_EINVAL, "offsets is NULL");
    if (!frame_offsets) return capi_fail(DSP_EINVAL, "frame_offsets is NULL");
    if (const int rc = dsp::check_frame_offsets(frame_offsets, n_clips, "clip")) return rc;
    if (from_signal)
        if (const int rc = check_rows(cfg, offsets, frame_offsets, n_clips)) return rc;
    for (long c = 0; c < n_clips; ++c)
        if (frame_offsets[c + 1] - frame_offsets[c] > INT32_MAX) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + " has 2^31 rows or more");
    Spans spans;
    spans.fill(from_signal ? offsets : nullptr, frame_offsets, n_clips);
    if (spans.rows == 0) {                                  // no row in the batch: no launch, and only kept_offsets is written
        if (decide) std::fill(kept_offsets, kept_offsets + n_clips + 1, 0L);
        return DSP_OK;
    }
    if (from_signal && !d_signal) return capi_fail(DSP_EINVAL, "d_signal is NULL");
    if (!keeps_power && !d_power) return capi_fail(DSP_EINVAL, "d_power is NULL");
    if (decide && !d_flags) return capi_fail(DSP_EINVAL, "d_flags is NULL");
    if (const int rc = check_workspace(d_workspace, workspace_bytes, dsp::vad_workspace_bytes(n_clips, spans.rows, keeps_power))) return rc;
    if (const int rc = dsp::check_device(device)) return rc;
    DSP_ON_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const dsp::VadWorkspace ws = dsp::vad_carve(d_workspace, n_clips, spans.rows, keeps_power);
    DSP_CAPI_HIP(spans.upload(ws, st));
    const size_t row0 = (size_t)frame_offsets[0];
    double *power = keeps_power ? ws.power : d_power ? d_power + row0 : nullptr;
    if (from_signal) DSP_CAPI_HIP(dsp::launch_vad_power(d_signal + offsets[0], ws, n_clips, spans.tiles, geo, cfg->frame_length, cfg->hop_length, power, st));
    if (!decide) return DSP_OK;
    DSP_CAPI_HIP(dsp::launch_vad_decide(power, ws, n_clips, spans.tiles, decision_of(cfg), d_flags ? d_flags + row0 : nullptr,
                                        d_level_db ? d_level_db + row0 : nullptr, d_clips, st));
    return download_kept_offsets(ws, n_clips, kept_offsets, st);
}

}  // namespace

extern "C" {

void dsp_vad_default_config(const dsp_mfcc_config *mfcc, dsp_vad_config *cfg)
{
    if (!cfg) return;
    *cfg = dsp_vad_config{};
    if (mfcc) {
        cfg->frame_length = mfcc->frame_length;
        cfg->hop_length = mfcc->hop_length;
        cfg->framing = mfcc->framing;
    }
    cfg->reference = DSP_VAD_REF_MAX;
    cfg->threshold_ratio = 1e-6;
    cfg->floor_power = 0.0;
    cfg->context_frames = 0;
    cfg->proportion = 0.6;
    cfg->pad_frames = 0;
}

double dsp_vad_ratio_from_db(double db) { return std::pow(10.0, db / 10.0); }

int dsp_vad_geometry_for(const dsp_vad_config *cfg, dsp_vad_geometry *out)
{
    dsp::VadGeometry geo;
    if (const int rc = check_config(cfg, geo)) return rc;
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    const long span = (long)(dsp::kVadTileRows - 1) * cfg->hop_length + cfg->frame_length;
    *out = dsp_vad_geometry{geo.g, geo.m, (int)std::min<long>(span, INT_MAX), dsp::kVadTileRows, cfg->context_frames + cfg->pad_frames};
    return DSP_OK;
}

long dsp_vad_workspace_bytes(long n_clips, long n_rows)
{
    if (n_clips < 0 || n_clips >= kMaxClips) return capi_fail(DSP_EINVAL, "n_clips must be 0 .. 2^31 - 1");
    if (n_rows < 0 || n_rows > (1L << 40)) return capi_fail(DSP_EINVAL, "n_rows must be 0 .. 2^40");
    return (long)dsp::vad_workspace_bytes(n_clips, n_rows, true);
}

int dsp_vad_frame_power_ragged_device(int device, const dsp_vad_config *cfg, const float *d_signal, long n_clips, const long *offsets,
                                      const long *frame_offsets, double *d_power, void *d_workspace, long workspace_bytes, void *stream)
{
    return vad_call(Call::Power, device, cfg, d_signal, d_power, n_clips, offsets, frame_offsets, nullptr, nullptr, nullptr, nullptr, d_workspace, workspace_bytes,
                    stream);
}

int dsp_vad_decide_ragged_device(int device, const dsp_vad_config *cfg, const double *d_power, long n_clips, const long *frame_offsets, uint8_t *d_flags,
                                 float *d_level_db, dsp_vad_clip *d_clips, long *kept_offsets, void *d_workspace, long workspace_bytes, void *stream)
{
    return vad_call(Call::Decide, device, cfg, nullptr, const_cast<double *>(d_power), n_clips, nullptr, frame_offsets, d_flags, d_level_db, d_clips, kept_offsets,
                    d_workspace, workspace_bytes, stream);
}

int dsp_vad_run_ragged_device(int device, const dsp_vad_config *cfg, const float *d_signal, long n_clips, const long *offsets, const long *frame_offsets,
                              uint8_t *d_flags, float *d_level_db, dsp_vad_clip *d_clips, long *kept_offsets, void *d_workspace, long workspace_bytes,
                              void *stream)
{
    return vad_call(Call::Run, device, cfg, d_signal, nullptr, n_clips, offsets, frame_offsets, d_flags, d_level_db, d_clips, kept_offsets, d_workspace,
                    workspace_bytes, stream);
}

int dsp_rows_kept_offsets_device(int device, const uint8_t *d_flags, long n_clips, const long *frame_offsets, long *kept_offsets, void *d_workspace,
                                 long workspace_bytes, void *stream)
{
    if (const int rc = check_call(device, n_clips)) return rc;
    if (!kept_offsets) return capi_fail(DSP_EINVAL, "kept_offsets is NULL");
    kept_offsets[0] = 0;
    if (n_clips == 0) return DSP_OK;
    if (!frame_offsets) return capi_fail(DSP_EINVAL, "frame_offsets is NULL");
    if (const int rc = dsp::check_frame_offsets(frame_offsets, n_clips, "clip")) return rc;
    Spans spans;
    spans.fill(nullptr, frame_offsets, n_clips);
    if (spans.rows == 0) {
        std::fill(kept_offsets, kept_offsets + n_clips + 1, 0L);
        return DSP_OK;
    }
    if (!d_flags) return capi_fail(DSP_EINVAL, "d_flags is NULL");
    if (const int rc = check_workspace(d_workspace, workspace_bytes, dsp::vad_workspace_bytes(n_clips, spans.rows, false))) return rc;
    if (const int rc = dsp::check_device(device)) return rc;
    DSP_ON_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const dsp::VadWorkspace ws = dsp::vad_carve(d_workspace, n_clips, spans.rows, false);
    DSP_CAPI_HIP(spans.upload(ws, st));
    DSP_CAPI_HIP(dsp::launch_rows_count(d_flags + frame_offsets[0], ws, n_clips, st));
    return download_kept_offsets(ws, n_clips, kept_offsets, st);
}

int dsp_rows_select_ragged_device(int device, const float *d_in, int d, const uint8_t *d_flags, long n_clips, const long *frame_offsets,
                                  const long *kept_offsets, float *d_out, long *d_row_index, void *d_workspace, long workspace_bytes, void *stream)
{
    if (const int rc = check_call(device, n_clips)) return rc;
    if (d < 1 || d > dsp::kVadMaxDim) return capi_fail(DSP_EINVAL, "d must be 1 .. 64, got " + std::to_string(d));
    if (n_clips == 0) return DSP_OK;
    if (!frame_offsets) return capi_fail(DSP_EINVAL, "frame_offsets is NULL");
    if (!kept_offsets) return capi_fail(DSP_EINVAL, "kept_offsets is NULL");
    if (const int rc = dsp::check_frame_offsets(frame_offsets, n_clips, "clip")) return rc;
    if (kept_offsets[0] != 0) return capi_fail(DSP_EINVAL, "kept_offsets must start at 0");
    for (long c = 0; c < n_clips; ++c) {
        const long kept = kept_offsets[c + 1] - kept_offsets[c];
        if (kept < 0) return capi_fail(DSP_EINVAL, "kept_offsets decrease at clip " + std::to_string(c));
        if (kept > frame_offsets[c + 1] - frame_offsets[c]) return capi_fail(DSP_EINVAL, "kept_offsets give clip " + std::to_string(c) + " more rows than it has");
    }
    const long rows = frame_offsets[n_clips] - frame_offsets[0], n_out = kept_offsets[n_clips];
    if (rows == 0 || n_out == 0) return DSP_OK;
    if (!d_in) return capi_fail(DSP_EINVAL, "d_in is NULL");
    if (!d_flags) return capi_fail(DSP_EINVAL, "d_flags is NULL");
    if (!d_out) return capi_fail(DSP_EINVAL, "d_out is NULL");
    const float *in = d_in + (size_t)frame_offsets[0] * (size_t)d;
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(in), in1 = in0 + (size_t)rows * d * sizeof(float);
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(d_out), out1 = out0 + (size_t)n_out * d * sizeof(float);
    if (out0 < in1 && in0 < out1) return capi_fail(DSP_EINVAL, "d_out overlaps the rows of d_in");
    if (const int rc = check_workspace(d_workspace, workspace_bytes, dsp::vad_workspace_bytes(n_clips, rows, false))) return rc;
    if (const int rc = dsp::check_device(device)) return rc;
    DSP_ON_DEVICE(device);
    const dsp::VadWorkspace ws = dsp::vad_carve(d_workspace, n_clips, rows, false);
    DSP_CAPI_HIP(dsp::launch_rows_select(in, d, d_flags + frame_offsets[0], rows, n_out, frame_offsets[0], ws, d_out, d_row_index, (hipStream_t)stream));
    return DSP_OK;
}

long dsp_vad_trim_spans(const dsp_vad_config *cfg, const long *offsets, long n_clips, const dsp_vad_clip *clips, long *starts, long *lengths)
{
    dsp::VadGeometry geo;
    if (const int rc = check_config(cfg, geo)) return rc;
    if (n_clips < 0) return capi_fail(DSP_EINVAL, "n_clips < 0");
    if (n_clips == 0) return 0;
    if (!offsets || !clips) return capi_fail(DSP_EINVAL, "offsets and clips must not be NULL");
    long with_speech = 0;
    for (long c = 0; c < n_clips; ++c) {
        const long n = dsp::ragged_clip_length(offsets, c);
        if (n < 0) return n;
        const dsp_vad_clip &r = clips[c];
        long a = 0, len = 0;
        if (r.n_kept > 0) {
            if (r.first_kept < 0 || r.last_kept < r.first_kept) return capi_fail(DSP_EINVAL, "clip " + std::to_string(c) + ": first_kept and last_kept are not a span");
            a = std::min(n, (long)r.first_kept * cfg->hop_length);
            len = std::min(n, ((long)r.last_kept + 1) * cfg->hop_length) - a;
            ++with_speech;
        }
        if (starts) starts[c] = offsets[c] + a;
        if (lengths) lengths[c] = len;
    }
    return with_speech;
}

}  // extern "C"
