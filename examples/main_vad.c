/*
 * main_vad.c -- drop the silence from recordings before a speaker is enrolled: the chain of INTEGRATION.md 6q in plain C.  Every
 * file of the command line is read as 16-bit mono PCM at 16 kHz and goes to the GPU once, as float32; there the recordings become one
 * ragged MFCC matrix of the rows the float GMMs are trained on (dsp_mfcc_speaker_config, dsp_mfcc_clips_ragged_device), are normalised
 * per recording (dsp_cmvn_ragged_device, window 300), and the voice activity detector keeps the rows whose frame power lies within
 * threshold_db of the recording's loudest frame (dsp_vad_run_ragged_device, dsp_rows_select_ragged_device: selection AFTER the CMVN,
 * Kaldi's order).  With a UBM the kept rows are MAP-adapted as ONE speaker (dsp_speaker_enroll_ragged_device).  The program prints,
 * per file, its rows, the rows kept and the span of samples librosa's trim would keep (dsp_vad_trim_spans).
 *
 *   gcc -O2 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/main_vad.c -Ldsp_amd -ldsp_amd -Wl,-rpath,$PWD/dsp_amd \
 *       -L/opt/rocm/lib -lamdhip64 -lm -o main_vad
 *   ./main_vad [-t threshold_db] [-c context_frames] [-p pad_frames] [-u ubm.txt] a.wav b.wav ...
 *
 * The float UBM is the text file examples/main_enroll.c reads: k d, then k log constants, k * d means, k * d inverse covariances.
 * Out of scope here: resampling (examples/main_enroll.c), stereo files.
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

/* appends the file's samples as float32 in [-1, 1) to *buf; returns the samples read, < 0 unless 16-bit mono PCM at 16 kHz */
static long read_wav_mono16k(const char *path, float **buf, long *used, long *cap)
{
    FILE *f = fopen(path, "rb");
    if (!f) return -1;
    uint8_t hdr[12];
    if (fread(hdr, 1, 12, f) != 12 || memcmp(hdr, "RIFF", 4) || memcmp(hdr + 8, "WAVE", 4)) { fclose(f); return -1; }
    int ch = 0, bits = 0, hz = 0;
    long n = -1;
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
            if (bits != 16 || ch != 1 || hz != 16000) break;
            const long count = (long)size / 2;
            if (*used + count > *cap) {
                *cap = 2 * (*used + count);
                *buf = (float *)realloc(*buf, (size_t)*cap * sizeof(float));
                if (!*buf) break;
            }
            long i = 0;
            for (; i < count; ++i) {
                uint8_t s[2];
                if (fread(s, 1, 2, f) != 2) break;
                (*buf)[*used + i] = (float)(int16_t)(s[0] | s[1] << 8) / 32768.0f;
            }
            if (i != count) break;
            *used += count;
            n = count;
            break;
        } else {
            fseek(f, (long)size + (size & 1), SEEK_CUR);
        }
    }
    fclose(f);
    return n;
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
    double threshold_db = -60.0;
    int context = 0, pad = 0, first = 1;
    const char *ubm_path = NULL;
    while (argc > first + 1 && argv[first][0] == '-' && argv[first][1] && !argv[first][2]) {
        const char opt = argv[first][1];
        if (opt == 't') threshold_db = atof(argv[first + 1]);
        else if (opt == 'c') context = atoi(argv[first + 1]);
        else if (opt == 'p') pad = atoi(argv[first + 1]);
        else if (opt == 'u') ubm_path = argv[first + 1];
        else break;
        first += 2;
    }
    const int n_files = argc - first;
    if (n_files <= 0 || argv[first][0] == '-') {
        fprintf(stderr, "usage: %s [-t threshold_db] [-c context_frames] [-p pad_frames] [-u ubm.txt] file.wav ...\n", argv[0]);
        return 2;
    }
    int k = 0, d = 0;
    double *ubm = NULL;
    if (ubm_path && !(ubm = read_ubm(ubm_path, &k, &d))) {
        fprintf(stderr, "%s: expected k d, k log constants, k * d means, k * d inverse covariances\n", ubm_path);
        return 1;
    }

    float *x = NULL;
    long used = 0, cap = 0;
    long *offsets = (long *)calloc((size_t)n_files + 1, sizeof(long)), *fo = (long *)calloc((size_t)n_files + 1, sizeof(long));
    long *kept = (long *)calloc((size_t)n_files + 1, sizeof(long)), *starts = (long *)calloc((size_t)n_files, sizeof(long));
    long *lengths = (long *)calloc((size_t)n_files, sizeof(long));
    dsp_vad_clip *clips = (dsp_vad_clip *)calloc((size_t)n_files, sizeof(dsp_vad_clip));
    if (!offsets || !fo || !kept || !starts || !lengths || !clips) { fprintf(stderr, "out of memory\n"); return 1; }
    for (int i = 0; i < n_files; ++i) {
        const long n = read_wav_mono16k(argv[first + i], &x, &used, &cap);
        if (n < 0) { fprintf(stderr, "%s: not a 16-bit mono PCM WAV at 16 kHz\n", argv[first + i]); return 1; }
        offsets[i + 1] = offsets[i] + n;
    }

    dsp_mfcc_config cfg;
    dsp_mfcc_speaker_config(&cfg);
    if (ubm && cfg.n_mfcc != d) { fprintf(stderr, "the UBM has d = %d, the MFCC front end %d coefficients\n", d, cfg.n_mfcc); return 1; }
    d = cfg.n_mfcc;
    dsp_vad_config vad;
    dsp_vad_default_config(&cfg, &vad);                    /* the plan's framing; reference = the recording's loudest frame */
    vad.threshold_ratio = dsp_vad_ratio_from_db(threshold_db);
    vad.context_frames = context;
    vad.pad_frames = pad;
    const long rows = dsp_mfcc_ragged_frame_offsets(&cfg, offsets, n_files, INT32_MAX, fo);
    DSP_OK_(rows);
    if (rows < 1) { fprintf(stderr, "the files hold no MFCC frame\n"); return 1; }
    const long ws_bytes = dsp_vad_workspace_bytes(n_files, rows);
    DSP_OK_(ws_bytes);

    dsp_mfcc_plan *plan = NULL;
    dsp_cmvn *cmvn = NULL;
    DSP_OK_(dsp_mfcc_plan_create(&cfg, 0, &plan));
    DSP_OK_(dsp_cmvn_create(0, d, 300, &cmvn));
    float *d_x = NULL, *d_mfcc = NULL, *d_feats = NULL, *d_speech = NULL;
    uint8_t *d_flags = NULL;
    dsp_vad_clip *d_clips = NULL;
    void *d_ws = NULL;
    HIP_OK(hipMalloc((void **)&d_x, (size_t)(used + 1) * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_mfcc, (size_t)rows * d * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_feats, (size_t)rows * d * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_speech, (size_t)rows * d * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_flags, (size_t)rows));
    HIP_OK(hipMalloc((void **)&d_clips, (size_t)n_files * sizeof(dsp_vad_clip)));
    HIP_OK(hipMalloc(&d_ws, (size_t)ws_bytes));
    HIP_OK(hipMemcpy(d_x, x, (size_t)used * sizeof(float), hipMemcpyHostToDevice));
    DSP_OK_(dsp_mfcc_clips_ragged_device(plan, d_x, n_files, offsets, INT32_MAX, d_mfcc, NULL));
    DSP_OK_(dsp_cmvn_ragged_device(cmvn, d_mfcc, n_files, fo, d_feats, NULL));
    /* the one wait of the chain: kept[] are host offsets, as every consumer takes them */
    DSP_OK_(dsp_vad_run_ragged_device(0, &vad, d_x, n_files, offsets, fo, d_flags, NULL, d_clips, kept, d_ws, ws_bytes, NULL));
    DSP_OK_(dsp_rows_select_ragged_device(0, d_feats, d, d_flags, n_files, fo, kept, d_speech, NULL, d_ws, ws_bytes, NULL));
    HIP_OK(hipMemcpy(clips, d_clips, (size_t)n_files * sizeof(dsp_vad_clip), hipMemcpyDeviceToHost));
    const long with_speech = dsp_vad_trim_spans(&vad, offsets, n_files, clips, starts, lengths);
    DSP_OK_(with_speech);
    for (int i = 0; i < n_files; ++i)
        printf("clip %d: %ld rows, %d kept, rows %d .. %d, samples [%ld, %ld) of %ld, threshold %.3e\n", i, fo[i + 1] - fo[i], clips[i].n_kept, clips[i].first_kept,
               clips[i].last_kept, starts[i] - offsets[i], starts[i] - offsets[i] + lengths[i], offsets[i + 1] - offsets[i], clips[i].threshold);
    printf("%ld of %d file(s) hold speech\n", with_speech, n_files);

    if (ubm) {
        if (kept[n_files] < 1) { fprintf(stderr, "no row is kept: nothing to enrol on\n"); return 1; }
        const dsp_gmm_float_params up = {k, d, ubm, ubm + k, ubm + k + k * d};
        const dsp_enroll_config ecfg = {DSP_MAP_RELEVANCE, 16.0f, 0.7f};
        dsp_speaker_enroller *en = NULL;
        float *d_ll = NULL, ll = 0.0f;
        int8_t *d_q6 = NULL;
        int *d_sat = NULL;
        DSP_OK_(dsp_speaker_enroller_create(&up, 0, &en));
        HIP_OK(hipMalloc((void **)&d_q6, (size_t)k * d));
        HIP_OK(hipMalloc((void **)&d_ll, sizeof(float)));
        HIP_OK(hipMalloc((void **)&d_sat, sizeof(int)));
        const long speaker[2] = {0, kept[n_files]};                                          /* all kept rows are one speaker */
        DSP_OK_(dsp_speaker_enroll_ragged_device(en, d_speech, 1, speaker, &ecfg, NULL, d_q6, NULL, d_ll, d_sat, NULL));
        HIP_OK(hipMemcpy(&ll, d_ll, sizeof(float), hipMemcpyDeviceToHost));
        printf("enrolled on %ld of %ld rows; mean log-likelihood under the UBM %.4f\n", kept[n_files], rows, ll);
        dsp_speaker_enroller_destroy(en);
        hipFree(d_q6); hipFree(d_ll); hipFree(d_sat);
    }

    dsp_cmvn_destroy(cmvn);
    dsp_mfcc_plan_destroy(plan);
    hipFree(d_x); hipFree(d_mfcc); hipFree(d_feats); hipFree(d_speech); hipFree(d_flags); hipFree(d_clips); hipFree(d_ws);
    free(x); free(offsets); free(fo); free(kept); free(starts); free(lengths); free(clips); free(ubm);
    return 0;
}
