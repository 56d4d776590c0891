// gmm_model.hpp -- the float32 diagonal GMM that the E-step of gmm_estep.hpp reads: one packed block, its limits and its packing.  Shared
// by enrolment (enroll_kernels.hpp: the UBM a speaker is adapted from) and by UBM training (ubm_kernels.hpp: the model of each iteration).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <vector>

namespace dsp {

constexpr int kGmmMaxK = 64, kGmmMaxD = 16;      // lane k of a wavefront owns component k; a row of features is staged at 16 floats

inline size_t gmm_model_floats(int k, int d) { return (size_t)k * (2 * d + 1); }      // log_consts[k] | means[k][d] | inv_covs[k][d], back to back

template <class F> struct GmmBlock {
    F *block;                // gmm_model_floats, on the device
    int k, d;
    __host__ __device__ F *log_consts() const { return block; }
    __host__ __device__ F *means() const { return block + k; }
    __host__ __device__ F *inv_covs() const { return block + k + (size_t)k * d; }
};
using GmmModel = GmmBlock<const float>;          // what an E-step reads
using GmmModelOut = GmmBlock<float>;             // what the M-step of UBM training writes for the next one

// the block on the host, each float64 value rounded once
inline std::vector<float> pack_gmm_model(int k, int d, const double *log_consts, const double *means, const double *inv_covs)
{
    std::vector<float> block(gmm_model_floats(k, d));
    const size_t kd = (size_t)k * d;
    for (int i = 0; i < k; ++i) block[(size_t)i] = (float)log_consts[i];
    for (size_t i = 0; i < kd; ++i) {
        block[(size_t)k + i] = (float)means[i];
        block[(size_t)k + kd + i] = (float)inv_covs[i];
    }
    return block;
}

}  // namespace dsp
