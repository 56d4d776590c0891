/*
 * main_segments.c -- where the stop word is said in long recordings: the chain of INTEGRATION.md 6b and 6j in plain C.  Every file of
 * the command line is read as 16-bit mono PCM at 16 kHz and goes to the GPU once; there the scanner turns the recordings into one
 * ragged MFCC matrix and P("stop") per sliding window (dsp_scanner_run_device: one second every 100 ms), and the segmenter turns the
 * windows into segments (dsp_segments_device: on at P >= 0.5, off below 0.3, gaps of up to 2 windows closed, fewer than 3 windows
 * dropped).  Only the segments come back to the host; dsp_segment_sample_spans gives each in samples, printed in seconds.
 *
 * The stop net is read from a text file: n_coef max_frames u0 u1 u2 u3, then scaler_mean and scaler_scale (n_coef * max_frames each),
 * then kernel and bias of each of the four layers, whitespace separated -- the arrays of the reference's model_params.h.
 *
 *   gcc -O2 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include examples/main_segments.c -Ldsp_amd -ldsp_amd -Wl,-rpath,$PWD/dsp_amd \
 *       -L/opt/rocm/lib -lamdhip64 -lm -o main_segments
 *   ./main_segments [-on 0.5] [-off 0.3] [-min 3] [-gap 2] stop_model.txt a.wav b.wav ...
 *
 * Out of scope here: other sample rates (examples/main_enroll.c resamples), stereo, the speaker scans (their scores go through the
 * same two calls with n_columns = speakers and DSP_SEG_EXCLUSIVE).
 */
#include <hip/hip_runtime_api.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsp_amd.h"

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)
#define DSP_OK_(call) do { if ((call) < 0) { fprintf(stderr, "%s: %s\n", #call, dsp_last_error()); return 1; } } while (0)

/* appends the file's samples as floats in [-1, 1) to *buf; returns samples read, < 0 on error */
static long read_wav_mono16(const char *path, float **buf, long *used, long *cap)
{
    FILE *f = fopen(path, "rb");
    if (!f) return -1;
    uint8_t hdr[12];
    if (fread(hdr, 1, 12, f) != 12 || memcmp(hdr, "RIFF", 4) || memcmp(hdr + 8, "WAVE", 4)) { fclose(f); return -1; }
    int ch = 1, bits = 16, hz = 0;
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
            n = (long)size / 2;
            if (*used + n > *cap) {
                *cap = 2 * (*used + n);
                *buf = (float *)realloc(*buf, (size_t)*cap * sizeof(float));
                if (!*buf) { n = -1; break; }
            }
            for (long i = 0; i < n; ++i) {
                uint8_t s[2];
                if (fread(s, 1, 2, f) != 2) { n = i; break; }
                (*buf)[*used + i] = (float)(int16_t)(s[0] | s[1] << 8) / 32768.0f;
            }
            *used += n;
            break;
        } else {
            fseek(f, (long)size + (size & 1), SEEK_CUR);
        }
    }
    fclose(f);
    return n;
}

static float *read_floats(FILE *f, long n)
{
    float *p = (float *)malloc((size_t)(n > 0 ? n : 1) * sizeof(float));
    for (long i = 0; p && i < n; ++i)
        if (fscanf(f, "%f", &p[i]) != 1) { free(p); return NULL; }
    return p;
}

int main(int argc, char **argv)
{
    dsp_segment_config seg_cfg = {0.5f, 0.3f, 3, 2, DSP_SEG_INDEPENDENT};
    int at = 1;
    for (; at + 1 < argc && argv[at][0] == '-'; at += 2) {
        if (!strcmp(argv[at], "-on")) seg_cfg.on = (float)atof(argv[at + 1]);
        else if (!strcmp(argv[at], "-off")) seg_cfg.off = (float)atof(argv[at + 1]);
        else if (!strcmp(argv[at], "-min")) seg_cfg.min_windows = atoi(argv[at + 1]);
        else if (!strcmp(argv[at], "-gap")) seg_cfg.max_gap = atoi(argv[at + 1]);
        else break;
    }
    if (argc - at < 2) {
        fprintf(stderr, "usage: %s [-on 0.5] [-off 0.3] [-min 3] [-gap 2] stop_model.txt a.wav b.wav ...\n", argv[0]);
        return 2;
    }
    /* the stop net */
    FILE *mf = fopen(argv[at], "r");
    dsp_stop_model_params sp;
    memset(&sp, 0, sizeof sp);
    if (!mf || fscanf(mf, "%d %d %d %d %d %d", &sp.n_coef, &sp.max_frames, &sp.units[0], &sp.units[1], &sp.units[2], &sp.units[3]) != 6 || sp.n_coef < 1 ||
        sp.max_frames < 1) {
        fprintf(stderr, "%s: not a stop model\n", argv[at]);
        return 1;
    }
    const long fan = (long)sp.n_coef * sp.max_frames;
    sp.scaler_mean = read_floats(mf, fan);
    sp.scaler_scale = read_floats(mf, fan);
    long in = fan;
    for (int l = 0; l < 4; ++l) {
        if (sp.units[l] < 1 || sp.units[l] > 16) { fprintf(stderr, "%s: layer %d has %d units\n", argv[at], l, sp.units[l]); return 1; }
        sp.kernel[l] = read_floats(mf, in * sp.units[l]);
        sp.bias[l] = read_floats(mf, sp.units[l]);
        if (!sp.kernel[l] || !sp.bias[l]) { fprintf(stderr, "%s: layer %d is cut short\n", argv[at], l); return 1; }
        in = sp.units[l];
    }
    fclose(mf);
    if (!sp.scaler_mean || !sp.scaler_scale) { fprintf(stderr, "%s: the scaler is cut short\n", argv[at]); return 1; }
    /* the recordings, back to back */
    const long n = argc - at - 1;
    long *offsets = (long *)calloc((size_t)n + 1, sizeof(long)), *fo = (long *)calloc((size_t)n + 1, sizeof(long)),
         *wo = (long *)calloc((size_t)n + 1, sizeof(long));
    float *signal = NULL;
    long used = 0, cap = 0;
    for (long r = 0; r < n; ++r) {
        if (read_wav_mono16(argv[at + 1 + r], &signal, &used, &cap) < 0) {
            fprintf(stderr, "%s: not a 16-bit mono WAV at 16 kHz\n", argv[at + 1 + r]);
            return 1;
        }
        offsets[r + 1] = used;
    }
    /* plan, net, scanner, segmenter */
    dsp_mfcc_config mfcc;
    dsp_mfcc_default_config(&mfcc);
    const dsp_scan_config scan = {98, 10};
    dsp_mfcc_plan *plan;
    dsp_stop_model *stop;
    dsp_scanner *scanner;
    dsp_segmenter *segmenter;
    DSP_OK_(dsp_mfcc_plan_create(&mfcc, 0, &plan));
    DSP_OK_(dsp_stop_model_create(&sp, 0, &stop));
    DSP_OK_(dsp_scanner_create(plan, stop, NULL, &scan, &scanner));
    DSP_OK_(dsp_segmenter_create(0, &segmenter));
    /* the layout, host only: rows per recording, windows per recording, the most segments there can be */
    DSP_OK_(dsp_mfcc_ragged_frame_offsets(&mfcc, offsets, n, INT_MAX, fo));
    const long windows = dsp_scan_window_offsets(&scan, fo, n, wo);
    DSP_OK_(windows);
    const long room = dsp_segments_capacity(&seg_cfg, wo, n, 1);
    DSP_OK_(room);
    float *d_signal, *d_prob;
    dsp_segment *d_segments;
    long *d_total;
    HIP_OK(hipMalloc((void **)&d_signal, (size_t)(used > 0 ? used : 1) * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_prob, (size_t)(windows > 0 ? windows : 1) * sizeof(float)));
    HIP_OK(hipMalloc((void **)&d_segments, (size_t)(room > 0 ? room : 1) * sizeof(dsp_segment)));
    HIP_OK(hipMalloc((void **)&d_total, 2 * sizeof(long)));
    HIP_OK(hipMemcpy(d_signal, signal, (size_t)used * sizeof(float), hipMemcpyHostToDevice));
    /* scan -> segments, on one stream, nothing waits in between */
    DSP_OK_(dsp_scanner_run_device(scanner, d_signal, n, offsets, d_prob, NULL, NULL, NULL));
    DSP_OK_(dsp_segments_device(segmenter, d_prob, n, wo, 1, &seg_cfg, d_segments, room, NULL, d_total, NULL));
    long total[2] = {0, 0};
    HIP_OK(hipMemcpy(total, d_total, sizeof total, hipMemcpyDeviceToHost));
    dsp_segment *segments = (dsp_segment *)malloc((size_t)(total[1] > 0 ? total[1] : 1) * sizeof(dsp_segment));
    long *starts = (long *)malloc((size_t)(total[1] > 0 ? total[1] : 1) * sizeof(long)), *lengths = (long *)malloc((size_t)(total[1] > 0 ? total[1] : 1) * sizeof(long));
    HIP_OK(hipMemcpy(segments, d_segments, (size_t)total[1] * sizeof(dsp_segment), hipMemcpyDeviceToHost));
    DSP_OK_(dsp_segment_sample_spans(&mfcc, &scan, offsets, n, segments, total[1], starts, lengths));
    printf("%ld windows, %ld segments\n", windows, total[0]);
    for (long i = 0; i < total[1]; ++i) {
        const dsp_segment *g = &segments[i];
        const double t0 = (double)(starts[i] - offsets[g->recording]) / mfcc.sample_rate, t1 = t0 + (double)lengths[i] / mfcc.sample_rate;
        printf("%s  %9.2f s .. %9.2f s  windows %d..%d  active %d  peak %.4f at window %d  mean %.4f\n", argv[at + 1 + g->recording], t0, t1, g->first_window,
               g->first_window + g->n_windows - 1, g->n_active, g->peak, g->peak_window, g->mean);
    }
    dsp_segmenter_destroy(segmenter);
    dsp_scanner_destroy(scanner);
    dsp_stop_model_destroy(stop);
    dsp_mfcc_plan_destroy(plan);
    (void)hipFree(d_signal); (void)hipFree(d_prob); (void)hipFree(d_segments); (void)hipFree(d_total);
    return 0;
}
