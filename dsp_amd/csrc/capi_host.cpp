// capi_host.cpp -- C ABI of the host pipeline (include/dsp_amd.h: dsp_host_*): pinned memory for C callers, the pipeline's configuration,
// what the last host call did, and the chunk planner.  The pipeline itself is host_pipe.hpp; the entries that run batches through it are
// capi.cpp's (MFCC) and classify_front.hpp's (both classifiers).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "host_pipe.hpp"

namespace host = dsp::host;
using dsp::capi_fail;

static int check_pipe_device(int device)
{
    return device >= 0 && device < dsp::kMaxDevices ? DSP_OK : capi_fail(DSP_EINVAL, "device index out of range");
}

extern "C" {

int dsp_host_alloc(int device, size_t bytes, void **out)
{
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    *out = nullptr;
    if (bytes == 0) return capi_fail(DSP_EINVAL, "bytes must be positive");
    if (device < 0) return capi_fail(DSP_EINVAL, "device index out of range");
    if (const int rc = dsp::check_device(device)) return rc;
    DSP_ON_DEVICE(device);
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return capi_fail(e == hipErrorOutOfMemory ? DSP_ENOMEM : DSP_EHIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    *out = p;
    return DSP_OK;
}

void dsp_host_free(void *p)
{
    if (p && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}

int dsp_host_pipeline_set(int device, const dsp_host_pipeline_config *cfg)
{
    if (const int rc = check_pipe_device(device)) return rc;
    if (cfg) {
        if (cfg->chunk_bytes < host::kMinChunkBytes) return capi_fail(DSP_EINVAL, "chunk_bytes must be at least 4096");
        if (cfg->depth < 1 || cfg->depth > host::kMaxDepth) return capi_fail(DSP_EINVAL, "depth must be 1 .. 4");
        if (cfg->pageable_mode < DSP_HOST_PAGEABLE_STAGE || cfg->pageable_mode > DSP_HOST_PAGEABLE_WHOLE)
            return capi_fail(DSP_EINVAL, "pageable_mode must be DSP_HOST_PAGEABLE_STAGE, _REGISTER, _DIRECT or _WHOLE");
        if (cfg->classify_min_clips < 1) return capi_fail(DSP_EINVAL, "classify_min_clips must be at least 1");
    }
    host::Pipe &pipe = host::pipes()[device];
    std::lock_guard<std::mutex> lock(pipe.mu);      // (no call is in flight under it: the entries are blocking)
    pipe.cfg = cfg ? *cfg : host::default_config();
    return DSP_OK;
}

int dsp_host_pipeline_get(int device, dsp_host_pipeline_config *cfg)
{
    if (const int rc = check_pipe_device(device)) return rc;
    if (!cfg) return capi_fail(DSP_EINVAL, "cfg is NULL");
    host::Pipe &pipe = host::pipes()[device];
    std::lock_guard<std::mutex> lock(pipe.mu);
    *cfg = pipe.cfg;
    return DSP_OK;
}

int dsp_host_pipeline_release(int device)
{
    if (const int rc = check_pipe_device(device)) return rc;
    host::Pipe &pipe = host::pipes()[device];
    std::lock_guard<std::mutex> lock(pipe.mu);
    if (pipe.device < 0) return DSP_OK;              // never opened: no device is touched
    DSP_ON_DEVICE(pipe.device);
    pipe.release();
    return DSP_OK;
}

int dsp_host_pipeline_stats(int device, dsp_host_stats *out)
{
    if (const int rc = check_pipe_device(device)) return rc;
    if (!out) return capi_fail(DSP_EINVAL, "out is NULL");
    host::Pipe &pipe = host::pipes()[device];
    std::lock_guard<std::mutex> lock(pipe.mu);
    *out = pipe.last;
    return DSP_OK;
}

long dsp_host_plan_chunks(long n_items, long item_bytes, const long *offsets, long chunk_bytes, long *first, long max_first)
{
    if (n_items < 0) return capi_fail(DSP_EINVAL, "n_items must not be negative");
    if (item_bytes < 1) return capi_fail(DSP_EINVAL, "item_bytes must be positive");
    if (chunk_bytes < host::kMinChunkBytes) return capi_fail(DSP_EINVAL, "chunk_bytes must be at least 4096");
    if (first && max_first < 1) return capi_fail(DSP_EINVAL, "max_first must be positive when first is given");
    std::vector<long> plan;
    if (offsets) {
        if (!host::plan_ragged(offsets, n_items, item_bytes, chunk_bytes, plan)) return capi_fail(DSP_EINVAL, "offsets must be non-decreasing");
        if (n_items == 0) plan.assign(1, 0);
    } else host::plan_uniform(n_items, item_bytes, chunk_bytes, plan);
    if (first) {
        if ((long)plan.size() > max_first) return capi_fail(DSP_EINVAL, "first has room for " + std::to_string(max_first) + " entries, the plan has " + std::to_string(plan.size()));
        for (size_t k = 0; k < plan.size(); ++k) first[k] = plan[k];
    }
    return (long)plan.size() - 1;
}

}  // extern "C"
