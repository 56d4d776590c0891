/*
 * main_enroll.c -- enrol one speaker from audio files: the chain of INTEGRATION.md 6e in plain C.  Every file of the command line is
 * read as 16-bit PCM (all at one sample rate, all mono or all stereo) and goes to the GPU once; there the recordings are resampled to
 * the models' 16 kHz (dsp_resample_ragged_pcm16_device), turned into one ragged MFCC matrix (dsp_mfcc_clips_ragged_device), normalised
 * per recording (dsp_cmvn_ragged_device, window 300) and MAP-adapted as ONE speaker against the float UBM
 * (dsp_speaker_enroll_ragged_device).  The program prints the target model's integer tables: the enrolled Q6 means, and the UBM's
 * log constants (Q8) and inverse covariances (Q11), which the target shares -- what dsp_speaker_model_create takes as `target`.
 *
 * The float UBM is read from a text file: k d, then k log constants, k * d means, k * d inverse covariances, whitespace separated.
 *
 *   gcc -O2 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/main_enroll.c -Ldsp_amd -ldsp_amd -Wl,-rpath,$PWD/dsp_amd \
 *       -L/opt/rocm/lib -lamdhip64 -lm -o main_enroll
 *   ./main_enroll [-l] [-a alpha | -r relevance] ubm.txt a.wav b.wav ...
 *
 * -l: the rows the reference's float GMMs are trained on (dsp_mfcc_speaker_config: librosa.feature.mfcc with n_fft 400, 128 mel filters,
 * centred frames; 2fa/audio/speaker/gmm_utils.py:52-58) instead of the firmware's 512-point front end (dsp_mfcc_default_config).
 *
 * Out of scope here: UBM training (examples/main_train_ubm.c).  Out of scope in the library too: variance or weight adaptation, CMVN for
 * live streams.
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

/* appends the file's samples (interleaved as stored) to *buf; returns sample frames read, < 0 on error */
static long read_wav_pcm16(const char *path, int16_t **buf, long *used, long *cap, int *channels, int *rate)
{
    FILE *f = fopen(path, "rb");
    if (!f) return -1;
    uint8_t hdr[12];
    if (fread(hdr, 1, 12, f) != 12 || memcmp(hdr, "RIFF", 4) || memcmp(hdr + 8, "WAVE", 4)) { fclose(f); return -1; }
    int ch = 1, bits = 16, hz = 0;
    long frames = -1;
    for (;;) {
        uint8_t ck[8];
        if (fread(ck, 1, 8, f) != 8) break;
        const uint32_t size = ck[4] | ck[5] << 8 | ck[6] << 16 | (uint32_t)ck[7] << 24;
        if (!memcmp(ck, "fmt ", 4)) {
            uint8_t fmt[16];
            if (size < 16 || fread(fmt, 1, 16, f) != 16) break;
            ch = fmt[2] | fmt[3] << 8;
            hz = (int)(fmt[4] | fmt[5] << 8 | fmt[6] << 16 | (uint32_t)fmt[7] << 24);
            bits = fmt[14] | fmt[15] << 8;
            fseek(f, (long)size - 16 + (size & 1), SEEK_CUR);
        } else if (!memcmp(ck, "data", 4)) {
            if (bits != 16 || (ch != 1 && ch != 2) || (*channels && (*channels != ch || *rate != hz))) break;
            *channels = ch;
            *rate = hz;
            const long n = (long)size / 2;
            if (*used + n > *cap) {
                *cap = 2 * (*used + n);
                *buf = (int16_t *)realloc(*buf, (size_t)*cap * sizeof(int16_t));
                if (!*buf) break;
            }
            if ((long)fread(*buf + *used, 2, (size_t)n, f) != n) break;
            *used += n;
            frames = n / ch;
            break;
        } else {
            fseek(f, (long)size + (size & 1), SEEK_CUR);
        }
    }
    fclose(f);
    return frames;
}

static double *read_ubm(const char *path, int *k, int *d)
{
    FILE *f = fopen(path, "r");
    if (!f) return NULL;
    double *v = NULL;
    if (fscanf(f, "%d %d", k, d) == 2 && *k >= 1 && *k <= 64 && *d >= 1 && *d <= 16) {
        const int n = *k * (2 * *d + 1);
        v = (double *)malloc((size_t)n * sizeof(double));
        for (int i = 0; v && i < n; ++i)
            if (fscanf(f, "%lf", &v[i]) != 1) { free(v); v = NULL; }
    }
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    dsp_enroll_config ecfg = {DSP_MAP_RELEVANCE, 16.0f, 0.7f};
    int first = 1, librosa_rows = 0;
    if (argc > 1 && !strcmp(argv[1], "-l")) { librosa_rows = 1; first = 2; }
    if (argc > first + 1 && !strcmp(argv[first], "-a")) { ecfg.map_mode = DSP_MAP_FIXED_ALPHA; ecfg.fixed_alpha = (float)atof(argv[first + 1]); first += 2; }
    else if (argc > first + 1 && !strcmp(argv[first], "-r")) { ecfg.relevance_factor = (float)atof(argv[first + 1]); first += 2; }
    const int n_files = argc - first - 1;
    if (n_files <= 0) { fprintf(stderr, "usage: %s [-l] [-a alpha | -r relevance] ubm.txt file.wav ...\n", argv[0]); return 2; }
    int k = 0, d = 0;
    double *ubm = read_ubm(argv[first], &k, &d);
    if (!ubm) { fprintf(stderr, "%s: expected k d, k log constants, k * d means, k * d inverse covariances\n", argv[first]); return 1; }
    const dsp_gmm_float_params up = {k, d, ubm, ubm + k, ubm + k + k * d};

    int16_t *pcm = NULL;
    long used = 0, cap = 0;
    int channels = 0, rate = 0;
    long *offsets = (long *)calloc((size_t)n_files + 1, sizeof(long));
    long *off16 = (long *)calloc((size_t)n_files + 1, sizeof(long)), *fo = (long *)calloc((size_t)n_files + 1, sizeof(long));
    int8_t *q6 = (int8_t *)malloc((size_t)k * d);
    if (!offsets || !off16 || !fo || !q6) { fprintf(stderr, "out of memory\n"); return 1; }
    for (int i = 0; i < n_files; ++i) {
        const long frames = read_wav_pcm16(argv[first + 1 + i], &pcm, &used, &cap, &channels, &rate);
        if (frames < 0) { fprintf(stderr, "%s: not a 16-bit PCM WAV (or its format differs from the files before it)\n", argv[first + 1 + i]); return 1; }
        offsets[i + 1] = offsets[i] + frames;
    }

    dsp_mfcc_config cfg;
    if (librosa_rows) dsp_mfcc_speaker_config(&cfg);
    else dsp_mfcc_default_config(&cfg);
    if (cfg.n_mfcc != d) { fprintf(stderr, "the UBM has d = %d, the MFCC front end %d coefficients\n", d, cfg.n_mfcc); return 1; }
    dsp_resampler *rs = NULL;
    dsp_mfcc_plan *plan = NULL;
    dsp_cmvn *cmvn = NULL;
    dsp_speaker_enroller *en = NULL;
    DSP_OK_(dsp_resampler_create(0, rate, cfg.sample_rate, &rs));
    DSP_OK_(dsp_mfcc_plan_create(&cfg, 0, &plan));
    DSP_OK_(dsp_cmvn_create(0, d, 300, &cmvn));
    DSP_OK_(dsp_speaker_enroller_create(&up, 0, &en));
    const long total16 = dsp_resample_offsets(rate, cfg.sample_rate, offsets, n_files, off16);
    DSP_OK_(total16);
    const long rows = dsp_mfcc_ragged_frame_offsets(&cfg, off16, n_files, INT32_MAX, fo);
    DSP_OK_(rows);
    if (rows < 1) { fprintf(stderr, "the files hold no complete MFCC frame\n"); return 1; }

    int16_t *d_pcm = NULL;
    int8_t *d_q6 = NULL;
    float *d_x16 = NULL, *d_mfcc = NULL, *d_feats = NULL, *d_ll = NULL;
    int *d_sat = NULL;
    HIP_OK(hipMalloc((void **)&d_pcm, (size_t)used * sizeof(int16_t)));
    HIP_OK(hipMalloc((void **)&d_x16, (size_t)(total16 + 1) * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_mfcc, (size_t)rows * d * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_feats, (size_t)rows * d * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_q6, (size_t)k * d));
    HIP_OK(hipMalloc((void **)&d_ll, sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_sat, sizeof(int)));
    HIP_OK(hipMemcpy(d_pcm, pcm, (size_t)used * sizeof(int16_t), hipMemcpyHostToDevice));
    /* four launches on the null stream, no host work between them */
    DSP_OK_(dsp_resample_ragged_pcm16_device(rs, d_pcm, n_files, offsets, channels, DSP_STEREO_CHANNEL0, d_x16, NULL));
    DSP_OK_(dsp_mfcc_clips_ragged_device(plan, d_x16, n_files, off16, INT32_MAX, d_mfcc, NULL));
    DSP_OK_(dsp_cmvn_ragged_device(cmvn, d_mfcc, n_files, fo, d_feats, NULL));                  /* each file is its own recording ... */
    const long speaker[2] = {fo[0], fo[n_files]};                                                /* ... and all of them are one speaker */
    DSP_OK_(dsp_speaker_enroll_ragged_device(en, d_feats, 1, speaker, &ecfg, NULL, d_q6, NULL, d_ll, d_sat, NULL));
    float ll = 0.0f;
    int sat = 0;
    HIP_OK(hipMemcpy(q6, d_q6, (size_t)k * d, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&ll, d_ll, sizeof(float), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&sat, d_sat, sizeof(int), hipMemcpyDeviceToHost));

    printf("/* enrolled from %d file(s), %ld rows; mean log-likelihood under the UBM %.4f; %d mean(s) saturated */\n", n_files, rows, ll, sat);
    printf("#define K %d\n#define D %d\n#define Q_LOG_CONSTS 8\n#define Q_MEANS 6\n#define Q_INV_COVS 11\n\n", k, d);
    printf("int16_t target_log_consts[K] = {\n");
    for (int i = 0; i < k; ++i) printf("    %ld,\n", lrint(ubm[i] * 256.0));
    printf("};\n\nint8_t target_means[K][D] = {\n");
    for (int i = 0; i < k; ++i) {
        printf("    {");
        for (int j = 0; j < d; ++j) printf("%d%s", q6[i * d + j], j + 1 < d ? ", " : "");
        printf("},\n");
    }
    printf("};\n\nint32_t target_inv_covs[K][D] = {\n");
    for (int i = 0; i < k; ++i) {
        printf("    {");
        for (int j = 0; j < d; ++j) printf("%ld%s", lrint(ubm[k + k * d + i * d + j] * 2048.0), j + 1 < d ? ", " : "");
        printf("},\n");
    }
    printf("};\n");

    dsp_speaker_enroller_destroy(en);
    dsp_cmvn_destroy(cmvn);
    dsp_mfcc_plan_destroy(plan);
    dsp_resampler_destroy(rs);
    hipFree(d_pcm); hipFree(d_x16); hipFree(d_mfcc); hipFree(d_feats); hipFree(d_q6); hipFree(d_ll); hipFree(d_sat);
    free(q6); free(pcm); free(offsets); free(off16); free(fo); free(ubm);
    return 0;
}
