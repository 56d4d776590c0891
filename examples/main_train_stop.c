/*
 * main_train_stop.c -- train the stop-word net behind classify_signal from labelled clips: the reference's keyword_classifier.py:155-232
 * (StandardScaler, Dense 4-2-2-1 with dropout, Adam, binary cross-entropy, EarlyStopping) in plain C.  The clips go
 * to the GPU once: dsp_mfcc_clips_device makes their MFCC matrices, dsp_stop_train_set_device fits the Scaler and standardises,
 * dsp_stop_train_runs_device trains all seeds side by side, the run with the lowest validation loss becomes a dsp_stop_model
 * (dsp_stop_model_from_training, dsp_stop_model_create) and dsp_classify_signal scores the clips with it.
 *
 * The clips here are synthetic one-second clips, noise with a two-tone burst in the ones labelled 1 (what tests/signals.py makes);
 * every fourth clip is held out for validation.
 *
 *   gcc -O2 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/main_train_stop.c -Ldsp_amd -ldsp_amd -Wl,-rpath,$PWD/dsp_amd \
 *       -L/opt/rocm/lib -lamdhip64 -lm -o main_train_stop
 *   ./main_train_stop [-n clips] [-s seeds] [-e epochs]
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsp_amd.h"

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)
#define DSP_OK_(call) do { if ((call) < 0) { fprintf(stderr, "%s: %s\n", #call, dsp_last_error()); return 1; } } while (0)
#define SAMPLES 16000
#define MAX_FRAMES 500

static const char *const kStatus[4] = {"stopped early", "ran every epoch", "no validation rows", "empty"};

int main(int argc, char **argv)
{
    int n = 48, n_seeds = 16, epochs = 40;
    for (int a = 1; a + 1 < argc; a += 2) {
        if (!strcmp(argv[a], "-n")) n = atoi(argv[a + 1]);
        else if (!strcmp(argv[a], "-s")) n_seeds = atoi(argv[a + 1]);
        else if (!strcmp(argv[a], "-e")) epochs = atoi(argv[a + 1]);
    }
    if (n < 8 || n > DSP_STOP_TRAIN_CAP_ROWS || n_seeds < 1 || n_seeds > DSP_STOP_TRAIN_CAP_RUNS || epochs < 1 || epochs > DSP_STOP_TRAIN_CAP_EPOCHS) {
        fprintf(stderr, "usage: %s [-n clips >= 8] [-s seeds] [-e epochs]\n", argv[0]);
        return 2;
    }
    /* clips and labels */
    float *clips = (float *)malloc((size_t)n * SAMPLES * sizeof(float));
    int *labels = (int *)malloc((size_t)n * sizeof(int)), *train_rows = (int *)malloc((size_t)n * sizeof(int)), *val_rows = (int *)malloc((size_t)n * sizeof(int));
    if (!clips || !labels || !train_rows || !val_rows) { fprintf(stderr, "out of memory\n"); return 1; }
    long n_train = 0, n_val = 0;
    uint64_t lcg = 1;
    for (int i = 0; i < n; ++i) {
        labels[i] = i & 1;
        if (i % 4 == 3 || i % 4 == 2) val_rows[n_val++] = i; else train_rows[n_train++] = i;
        const double t0 = 0.2 + 0.005 * i, t1 = t0 + 0.4;
        for (int k = 0; k < SAMPLES; ++k) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            const double t = k / 16000.0, noise = 0.05 * ((double)(lcg >> 40) / (double)(1 << 23) - 1.0);
            const double tone = labels[i] && t >= t0 && t < t1 ? 0.3 * sin(2 * M_PI * 700.0 * t) + 0.2 * sin(2 * M_PI * 1900.0 * t) : 0.0;
            clips[(size_t)i * SAMPLES + k] = (float)(noise + tone);
        }
    }

    /* clips -> MFCC matrices, frame-major [n][T][13] */
    dsp_mfcc_config cfg;
    dsp_mfcc_default_config(&cfg);
    dsp_mfcc_plan *plan = NULL;
    DSP_OK_(dsp_mfcc_plan_create(&cfg, 0, &plan));
    const int T = dsp_mfcc_frames_for(&cfg, SAMPLES, MAX_FRAMES), n_coef = cfg.n_mfcc;
    float *d_clips = NULL, *d_mfcc = NULL;
    HIP_OK(hipMalloc((void **)&d_clips, (size_t)n * SAMPLES * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_mfcc, (size_t)n * T * n_coef * sizeof(float)));
    HIP_OK(hipMemcpy(d_clips, clips, (size_t)n * SAMPLES * sizeof(float), hipMemcpyHostToDevice));
    DSP_OK_(dsp_mfcc_clips_device(plan, d_clips, n, SAMPLES, SAMPLES, d_mfcc, MAX_FRAMES, NULL));

    /* the dataset: the Scaler is fitted on the training clips */
    const int units[4] = {4, 2, 2, 1};
    const long n_in = (long)n_coef * MAX_FRAMES, n_params = dsp_stop_train_param_count(n_coef, MAX_FRAMES, units);
    long *frame_offsets = (long *)malloc((size_t)(n + 1) * sizeof(long));
    float *mean = (float *)malloc((size_t)n_in * sizeof(float)), *scale = (float *)malloc((size_t)n_in * sizeof(float));
    if (!frame_offsets || !mean || !scale || n_params < 0) { fprintf(stderr, "out of memory\n"); return 1; }
    for (int i = 0; i <= n; ++i) frame_offsets[i] = (long)i * T;
    dsp_stop_trainer *trainer = NULL;
    DSP_OK_(dsp_stop_trainer_create(0, n_coef, MAX_FRAMES, units, &trainer));
    DSP_OK_(dsp_stop_train_set_device(trainer, d_mfcc, n, frame_offsets, train_rows, n_train, NULL, NULL, mean, scale, NULL));

    /* one run per seed, all in one call */
    dsp_stop_train_run *runs = (dsp_stop_train_run *)calloc((size_t)n_seeds, sizeof(*runs));
    dsp_stop_train_result *results = (dsp_stop_train_result *)calloc((size_t)n_seeds, sizeof(*results));
    if (!runs || !results) { fprintf(stderr, "out of memory\n"); return 1; }
    for (int s = 0; s < n_seeds; ++s) {
        const dsp_stop_train_run r = {train_rows, val_rows, n_train, n_val, (unsigned long long)s, 1e-2, {0.1, 0.1, 0.0}, 8, epochs, 10, 1};
        runs[s] = r;
    }
    double *d_history = NULL, *d_params = NULL;
    HIP_OK(hipMalloc((void **)&d_history, (size_t)n_seeds * epochs * 2 * sizeof(double)));
    HIP_OK(hipMalloc((void **)&d_params, (size_t)n_seeds * n_params * sizeof(double)));
    DSP_OK_(dsp_stop_train_runs_device(trainer, runs, n_seeds, labels, results, d_history, NULL, d_params, NULL));
    int best = -1, dead = 0;
    for (int s = 0; s < n_seeds; ++s) {
        printf("seed %2d: %3d epochs (%s), best epoch %3d, val_loss %.6f, %d of %ld validation clips right, %d dead units\n", s, results[s].n_epochs,
               kStatus[results[s].status], results[s].best_epoch, results[s].best_val_loss, results[s].val_correct, n_val, results[s].n_dead_units);
        dead += results[s].n_dead_units > 0;
        if (results[s].best_val_loss == results[s].best_val_loss && (best < 0 || results[s].best_val_loss < results[best].best_val_loss)) best = s;
    }
    if (best < 0) { fprintf(stderr, "no run has a validation loss\n"); return 1; }
    printf("%d of %d seeds lost units; keeping seed %d\n", dead, n_seeds, best);

    /* the best run as a model, and classify_signal on every clip */
    double *params = (double *)malloc((size_t)n_params * sizeof(double));
    float *arrays = (float *)malloc((size_t)(2 * n_in + n_params) * sizeof(float));
    if (!params || !arrays) { fprintf(stderr, "out of memory\n"); return 1; }
    HIP_OK(hipMemcpy(params, d_params + (size_t)best * n_params, (size_t)n_params * sizeof(double), hipMemcpyDeviceToHost));
    dsp_stop_model_params mp;
    DSP_OK_(dsp_stop_model_from_training(n_coef, MAX_FRAMES, units, params, mean, scale, arrays, &mp));
    dsp_stop_model *model = NULL;
    DSP_OK_(dsp_stop_model_create(&mp, 0, &model));
    int right = 0;
    for (int i = 0; i < n; ++i) {
        const float p = dsp_classify_signal(model, clips + (size_t)i * SAMPLES, SAMPLES);
        right += (p > 0.5f) == (labels[i] == 1);
    }
    printf("classify_signal: %d of %d clips right\n", right, n);

    dsp_stop_model_destroy(model);
    dsp_stop_trainer_destroy(trainer);
    dsp_mfcc_plan_destroy(plan);
    hipFree(d_history); hipFree(d_params); hipFree(d_mfcc); hipFree(d_clips);
    free(arrays); free(params); free(results); free(runs); free(scale); free(mean); free(frame_offsets); free(val_rows); free(train_rows); free(labels); free(clips);
    return right == n ? 0 : 3;
}
