// stream_load.hpp -- the cache policy of a global load, chosen at COMPILE time.
//
//   load_stream(p)            non-temporal (`global_load_* ... nt`): data that is read exactly once (back-to-back frames);
//                             nothing useful is displaced in L2 / MALL and the walk costs less energy per byte
//   load_cached(p)            plain load: data that is read again soon (overlapping frames of a clip)
//   load_frame_word<STREAM>   one or the other by a template constant
//
// The choice must never be a run-time value, not even one that is constant in every instantiation:
// `flag ? __builtin_nontemporal_load(p) : *p` is two loads of one address, the optimiser merges them into one and the merged
// load keeps only the metadata both had -- the !nontemporal hint is gone and the binary reads cacheable (this is how the
// 512-point, the general 1024-point and the 2048-point kernels lost it).  `if constexpr` leaves one load per
// instantiation.  tests/test_stream_loads_cpu.py checks the built code object, tools/stream_loads.py prints it.
#pragma once

namespace dsp {

template <typename V>
__device__ __forceinline__ V load_stream(const V *p) { return __builtin_nontemporal_load(p); }

template <typename V>
__device__ __forceinline__ V load_cached(const V *p) { return *p; }

template <bool STREAM, typename V>
__device__ __forceinline__ V load_frame_word(const V *p)
{
    if constexpr (STREAM) return load_stream(p);
    else return load_cached(p);
}

}  // namespace dsp
