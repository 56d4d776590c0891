/*
 * main_train_ubm.c -- train the speaker UBM from feature rows: the reference's
 * GaussianMixture(n_components=32, covariance_type="diag", max_iter=300, n_init=2).fit(rows) of 2fa/audio/speaker/train_ubm.py in plain
 * C.  The rows go to the GPU once; there dsp_kmeans_train_ubm_device seeds (k-means++), runs Lloyd, starts EM from the
 * GMM of the labels -- twice, keeping the better fit -- and dsp_gmm_quantize turns the float UBM into the integer scorer's tables.  No
 * host pass lies between the feature matrix and the tables.
 *
 * The rows are read from a text file: n d, then n * d values, whitespace separated (CMVN'd MFCC rows of all recordings, stacked; from
 * audio they come as in main_enroll.c).  Printed: what each restart did, then the tables as C arrays.
 *
 *   gcc -O2 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/main_train_ubm.c -Ldsp_amd -ldsp_amd -Wl,-rpath,$PWD/dsp_amd \
 *       -L/opt/rocm/lib -lamdhip64 -lm -o main_train_ubm
 *   ./main_train_ubm [-k components] [-s seed] [-n n_init] rows.txt
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsp_amd.h"

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)
#define DSP_OK_(call) do { if ((call) < 0) { fprintf(stderr, "%s: %s\n", #call, dsp_last_error()); return 1; } } while (0)

static const char *const kStop[3] = {"max_iter", "tol", "strict"};

int main(int argc, char **argv)
{
    int k = 32, first = 1;
    dsp_kmeans_ubm_config cfg = {2, 0, 300, 1e-4, {300, 1e-3, 1e-6}};      /* train_ubm.py: n_init 2, max_iter 300; sklearn's defaults otherwise */
    while (argc > first + 1 && argv[first][0] == '-') {
        if (!strcmp(argv[first], "-k")) k = atoi(argv[first + 1]);
        else if (!strcmp(argv[first], "-s")) cfg.seed = strtoull(argv[first + 1], NULL, 10);
        else if (!strcmp(argv[first], "-n")) cfg.n_init = atoi(argv[first + 1]);
        else break;
        first += 2;
    }
    if (argc != first + 1 || cfg.n_init < 1 || cfg.n_init > 64) { fprintf(stderr, "usage: %s [-k components] [-s seed] [-n n_init] rows.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[first], "r");
    long n = 0;
    int d = 0;
    if (!f || fscanf(f, "%ld %d", &n, &d) != 2 || n < 1 || d < 1 || d > 16) { fprintf(stderr, "%s: expected n d, then n * d values\n", argv[first]); return 1; }
    float *rows = (float *)malloc((size_t)n * d * sizeof(float));
    if (!rows) { fprintf(stderr, "out of memory\n"); return 1; }
    for (long i = 0; i < n * d; ++i)
        if (fscanf(f, "%f", &rows[i]) != 1) { fprintf(stderr, "%s: value %ld is missing\n", argv[first], i); return 1; }
    fclose(f);

    dsp_ubm_trainer *trainer = NULL;
    DSP_OK_(dsp_ubm_trainer_create(0, k, d, &trainer));
    float *d_rows = NULL;
    HIP_OK(hipMalloc((void **)&d_rows, (size_t)n * d * sizeof(float)));
    HIP_OK(hipMemcpy(d_rows, rows, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice));

    const size_t kd = (size_t)k * d;
    double *buf = (double *)calloc(2 * (size_t)k + 3 * kd + (size_t)cfg.em.max_iter, sizeof(double));
    dsp_kmeans_restart restarts[64];
    if (!buf) { fprintf(stderr, "out of memory\n"); return 1; }
    dsp_ubm_result res;
    memset(&res, 0, sizeof(res));
    res.gmm.log_consts = buf;
    res.gmm.means = buf + k;
    res.gmm.inv_covs = buf + k + kd;
    res.weights = buf + k + 2 * kd;
    res.variances = buf + 2 * (size_t)k + 2 * kd;
    res.lower_bounds = buf + 2 * (size_t)k + 3 * kd;
    dsp_kmeans_ubm_report report = {restarts, -1};
    DSP_OK_(dsp_kmeans_train_ubm_device(trainer, d_rows, n, &cfg, &res, &report, NULL));

    int8_t *q_means = (int8_t *)malloc(kd);
    int32_t *q_inv_covs = (int32_t *)malloc(kd * sizeof(int32_t));
    int16_t *q_log_consts = (int16_t *)malloc((size_t)k * sizeof(int16_t));
    int saturated[3];
    if (!q_means || !q_inv_covs || !q_log_consts) { fprintf(stderr, "out of memory\n"); return 1; }
    DSP_OK_(dsp_gmm_quantize(&res.gmm, q_means, q_inv_covs, q_log_consts, saturated));

    printf("/* UBM of %d components from %ld rows x %d, seed %llu\n", k, n, d, (unsigned long long)cfg.seed);
    for (int r = 0; r < cfg.n_init; ++r)
        printf(" * restart %d: first seed row %ld, k-means %d iterations (%s, %d empty), EM %d iterations%s, lower bound %.9f%s\n", r, restarts[r].rows[0],
               restarts[r].kmeans_n_iter, kStop[restarts[r].kmeans_stop], restarts[r].kmeans_n_empty, restarts[r].em_n_iter,
               restarts[r].em_converged ? " (converged)" : "", restarts[r].lower_bound, r == report.winner ? "  <- kept" : "");
    printf(" * clamped: %d mean(s), %d inverse covariance(s), %d log constant(s) */\n", saturated[0], saturated[1], saturated[2]);
    printf("#define K %d\n#define D %d\n#define Q_LOG_CONSTS 8\n#define Q_MEANS 6\n#define Q_INV_COVS 11\n\n", k, d);
    printf("int16_t ubm_log_consts[K] = {\n");
    for (int i = 0; i < k; ++i) printf("    %d,\n", q_log_consts[i]);
    printf("};\n\nint8_t ubm_means[K][D] = {\n");
    for (int i = 0; i < k; ++i) {
        printf("    {");
        for (int j = 0; j < d; ++j) printf("%d%s", q_means[i * d + j], j + 1 < d ? ", " : "");
        printf("},\n");
    }
    printf("};\n\nint32_t ubm_inv_covs[K][D] = {\n");
    for (int i = 0; i < k; ++i) {
        printf("    {");
        for (int j = 0; j < d; ++j) printf("%d%s", q_inv_covs[i * d + j], j + 1 < d ? ", " : "");
        printf("},\n");
    }
    printf("};\n");

    dsp_ubm_trainer_destroy(trainer);
    hipFree(d_rows);
    free(q_means); free(q_inv_covs); free(q_log_consts); free(buf); free(rows);
    return 0;
}
