// kmeans_kernels.hpp -- the start of UBM training: greedy k-means++ seeding, Lloyd iterations and the GMM they leave (include/dsp_amd.h
// dsp_kmeans_*): what the host code of capi_ubm.cpp hands the kernels of kmeans_kernels.hip.  The reduction tree is
// the one of ubm_kernels.hpp, a function of the row count alone.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "gmm_model.hpp"
#include "ubm_kernels.hpp"

namespace dsp {

constexpr int kKmeansMaxTrials = 6;              // 2 + floor(ln 64)
constexpr int kKmeansSegmentRows = 16;           // a chunk's float64 sum of the seeding: 16 segments of 16 rows, ascending in and across them
inline long kmeans_chunks(long n) { return (n + kUbmChunkRows - 1) / kUbmChunkRows; }

// --- Lloyd ---
// one partial: [k][2 d + 1] doubles (N_k, F_k[0..d), G_k[0..d)), then the inertia and the number of rows whose label changed
inline size_t kmeans_partial_doubles(int k, int d) { return (size_t)k * (2 * d + 1) + 2; }

enum KmeansStop { kKmeansStopMaxIter = 0, kKmeansStopTol = 1, kKmeansStopStrict = 2 };

// `done` is tested first by every kernel of every later iteration
struct KmeansCtrl {
    int done, reason, n_iter, n_empty;
    double inertia;          // of the final pass
};

struct KmeansFit {
    const float *feats;      // [n][d]
    long n;
    double *centres;         // [k][d], float64 between iterations
    GmmModelOut model;       // means(): c = float32(centre) of the next iteration; the final pass writes the whole E-step model of the GMM start
    int *labels;             // [n]: the previous iteration's on the way in (-1 before the first), this one's on the way out
    double *groups, *supers; // [ubm_groups(n)] and [ubm_supers(n)] partials
    KmeansCtrl *ctrl;
    double shift_limit;      // tol * mean_d var_d(x)
    int max_iter;
    double reg_covar;
    double *params;          // ubm_param_doubles: the GMM start (final pass)
    double *counts;          // [k]: N_k of the final pass
};

// iterations [first, first + count) of Lloyd: per iteration the labelled statistics, the supers and the update of the centres
hipError_t launch_kmeans_iterations(const KmeansFit &fit, int first, int count, hipStream_t stream);
// the pass after the stop: labels against the final centres, N, F, G -> the M-step of dsp_amd.h step 4 into params and the float32 model
hipError_t launch_kmeans_final(const KmeansFit &fit, hipStream_t stream);

// --- seeding ---
struct KmeansSeedCtrl {
    int failed;              // 1: the potential reached 0 with centres left to choose (fewer than k distinct rows)
    int failed_step;
    long rows[kGmmMaxK];     // the chosen rows, in the order chosen
    long cand[kKmeansMaxTrials];      // the proposals of the step about to be evaluated
    double pot[kGmmMaxK];    // the potential after each choice
};

struct KmeansSeed {
    const float *feats;
    long n;
    int k, d, trials;
    float *m;                // [n]: the squared distance to the nearest chosen centre
    double *chunks;          // [trials][kmeans_chunks(n)]
    double *groups;          // [trials][ubm_groups(n)]
    double *supers;          // [trials][ubm_supers(n)]
    const double *u;         // [k][kKmeansMaxTrials]: the draws u(seed, j, t), uploaded by the host
    KmeansSeedCtrl *ctrl;
};

// all k steps: per step one pass over the rows and one single-block kernel that picks the winner and the next proposals
hipError_t launch_kmeans_seeding(const KmeansSeed &seed, long row0, hipStream_t stream);

// the counter-based draws of include/dsp_amd.h (host): splitmix64's finaliser
inline uint64_t kmeans_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline double kmeans_draw(uint64_t seed, int j, int t) { return (double)(kmeans_mix(seed + (uint64_t)(8 * j + t + 1) * 0x9E3779B97F4A7C15ull) >> 11) * 0x1.0p-53; }
inline uint64_t kmeans_restart_seed(uint64_t seed, int r) { return kmeans_mix((seed ^ 0xD1B54A32D192ED03ull) + (uint64_t)(r + 1) * 0x9E3779B97F4A7C15ull); }
inline int kmeans_trials(int k)
{
    int t = 2;                                   // 2 + floor(ln k) without a call of log: e^1 .. e^4 = 2.72, 7.39, 20.09, 54.6
    for (int bound : {3, 8, 21, 55}) t += k >= bound;
    return t;
}

}  // namespace dsp
