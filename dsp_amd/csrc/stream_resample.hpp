// stream_resample.hpp -- what a stream session (capi_stream.cpp) needs to know of a streaming resampler (capi_resample.cpp,
// include/dsp_amd.h dsp_stream_resample*) that stands in front of it.  Host only, internal.
#pragma once

#include "../../include/dsp_amd.h"

namespace dsp {

struct StreamResamplerInfo {
    int device, rate_out;
    long n_streams;
};
StreamResamplerInfo stream_resampler_info(const dsp_stream_resampler *rs);

// what the resampler's next push of these chunks would emit: out_offsets[n_streams + 1] from its own counters; the total or < 0.
// Changes nothing.
long stream_resampler_plan(dsp_stream_resampler *rs, const long *chunk_offsets, long *out_offsets);

// a HIP call failed behind the first launch of one of its pushes
bool stream_resampler_broken(dsp_stream_resampler *rs);

}  // namespace dsp
