// svmtrain_kernels.hpp -- training the scrub-jay RBF-SVM on the GPU (include/dsp_amd.h dsp_svm_train_*): the kernels'
// constants, what a problem looks like on the device and what capi_svmtrain.cpp hands the kernels of svmtrain_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/dsp_amd.h"

namespace dsp {

constexpr long kSvmTrainMaxRows = 8192;            // D2 is n x n float64: 512 MB at the cap
constexpr int kSvmTrainBlock = 256;                // the solver's workgroup: one wavefront per SIMD
constexpr int kSvmTrainMaxIter = 100000000;
constexpr int kSvmTrainDefaultIter = 1000000;
constexpr int kSvmPlattMaxIter = 100;

// One problem as the solver reads it.  members[first .. first + n_members) are its rows of the shared matrix, strictly ascending.
// `status` is what the host already knows (DSP_SVM_TRAIN_ONE_CLASS / _EMPTY: the solver does not run, `fill` is the decision of every
// row) or DSP_SVM_TRAIN_CONVERGED: run.
struct SvmTrainProblem {
    long first;
    int n_members, status;
    double c[2];                                   // the box bound of label 0, label 1
    double gamma;
    double fill;
};
static_assert(sizeof(SvmTrainProblem) == 48, "a problem is 48 bytes");

// the solver's dynamic LDS: gradient and alpha as doubles, then the members' y as bytes
inline size_t svm_smo_lds_bytes(int n_members) { return (size_t)n_members * 17 + 16; }

struct SvmPlattOut { double a, b; int n_iter, reserved; };

// offset[f] = mean, scale[f] = 1 / std (std 0: 1) of feature f over rows[0 .. n_rows) (nullptr: rows 0 .. n_rows - 1), float64 sums
hipError_t launch_svm_scaler_fit(const float *feat, int n_features, const int *rows, long n_rows, float *offset, float *scale, hipStream_t stream);
// z = fl32(fl32(x - offset) * scale), then D2[i][j] = sum_f ((double)z_if - (double)z_jf)^2, features ascending
hipError_t launch_svm_distances(const float *feat, long n, int n_features, const float *offset, const float *scale, float *z, double *d2,
                                hipStream_t stream);
// one workgroup per problem (q_float32: the solver's kernel values rounded to float32, libsvm's Qfloat), its LDS sized for the launch's largest problem (max_members); coef[P][n] must be zero on entry
hipError_t launch_svm_smo(const double *d2, long n, const int *members, const SvmTrainProblem *problems, long n_problems, int max_members,
                          const int *labels, double eps, int max_iter, int q_float32, double *coef, dsp_svm_train_result *results, hipStream_t stream);
// dec[P][n]: every row's decision under every problem (nullptr: not wanted)
hipError_t launch_svm_decisions(const double *d2, long n, const int *members, const SvmTrainProblem *problems, long n_problems,
                                const double *coef, const dsp_svm_train_result *results, double *dec, hipStream_t stream);
// dec_cv[i] = dec[fold_ids[i]][i]
hipError_t launch_svm_gather_cv(const double *dec, long n, const int *fold_ids, double *dec_cv, hipStream_t stream);
// libsvm's sigmoid_train on (dec[rows[k]], labels[rows[k]]), one block
hipError_t launch_svm_platt(const double *dec, const int *labels, const int *rows, long n_rows, SvmPlattOut *out, hipStream_t stream);

}  // namespace dsp
