/* oracle_coupling.c -- the oracle's channel coupling on the records of tests/edge_coupling.py, as a process of its own
 * so that it can be built with AddressSanitizer + UBSan (tests/test_coupling_reach.py links it with oracle/ *.c).  What
 * the GPU parity test compares against must be defined behaviour of the restated reference, not an out-of-range read.
 *
 * Input file: runs, one after the other, each
 *   int32 kind, channels, n, k, form, s16
 *   kind 0 (dependent coupling, k = n_cce; form 0: TOOLS_ALL, 1: TOOLS_PRE then TOOLS_POST, 2: TOOLS_POST alone):
 *     int32 rng [n], float coeffs [n][channels][1024], HeaacToolsFrame [n], HeaacCceFrame [n][k],
 *     float cce_coeffs [n][k][1024]
 *   kind 1 (independent coupling, k chained calls on one target, int16 output when s16):
 *     float pcm [n][channels][1024], then per call float cce [n][1024], HeaacCoupling [n]
 * Output: one line per run (with the number of NaN words the run leaves) and "ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "oracle.h"

static void *take(FILE *f, size_t bytes)
{
    void *p = malloc(bytes ? bytes : 1);
    if (!p || fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "short file\n"); exit(2); }
    return p;
}

static long nans(const float *a, size_t words)
{
    long c = 0;
    for (size_t i = 0; i < words; i++) c += isnan(a[i]) != 0;
    return c;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: oracle_coupling records.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[6];
    int runs = 0;
    long frames = 0;
    while (fread(head, sizeof(head), 1, f) == 1) {
        const int kind = head[0], channels = head[1], n = head[2], k = head[3], form = head[4], s16 = head[5];
        if ((channels != 1 && channels != 2) || n < 1 || k < 1 || kind < 0 || kind > 1 || form < 0 || form > 2) {
            fprintf(stderr, "bad run header\n");
            return 2;
        }
        const size_t words = (size_t)n * channels * 1024;
        long bad;
        if (kind == 0) {
            int32_t *rng = take(f, (size_t)n * sizeof(*rng));
            float *coeffs = take(f, words * sizeof(float));
            HeaacToolsFrame *tools = take(f, (size_t)n * sizeof(*tools));
            HeaacCceFrame *cce = take(f, (size_t)n * k * sizeof(*cce));
            float *cc = take(f, (size_t)n * k * 1024 * sizeof(float));
            if (form == 0) {
                oracle_spectral_tools_batch_ex(channels, HEAAC_TOOLS_ALL, coeffs, tools, rng, rng, NULL, NULL, cce, cc, k,
                                               (size_t)n);
            } else if (form == 1) {
                oracle_spectral_tools_batch_ex(channels, HEAAC_TOOLS_PRE, coeffs, tools, rng, rng, NULL, NULL, NULL, NULL,
                                               0, (size_t)n);
                oracle_spectral_tools_batch_ex(channels, HEAAC_TOOLS_POST, coeffs, tools, NULL, NULL, NULL, NULL, cce, cc,
                                               k, (size_t)n);
            } else {
                oracle_spectral_tools_batch_ex(channels, HEAAC_TOOLS_POST, coeffs, tools, rng, rng, NULL, NULL, cce, cc, k,
                                               (size_t)n);
            }
            bad = nans(coeffs, words);
            free(rng); free(coeffs); free(tools); free(cce); free(cc);
        } else {
            float *pcm = take(f, words * sizeof(float));
            int16_t *o16 = s16 ? malloc(words * sizeof(*o16)) : NULL;
            for (int call = 0; call < k; call++) {
                float *cce = take(f, (size_t)n * 1024 * sizeof(float));
                HeaacCoupling *cpl = take(f, (size_t)n * sizeof(*cpl));
                if (oracle_couple_after_imdct_batch(channels, pcm, cce, cpl, o16, (size_t)n)) return 1;
                free(cce); free(cpl);
            }
            bad = nans(pcm, words);
            free(pcm); free(o16);
        }
        printf("run %d: kind %d, %d channels, %d frames, k %d, form %d: %ld NaN words\n", runs, kind, channels, n, k, form,
               bad);
        frames += n;
        runs++;
    }
    fclose(f);
    printf("runs %d, frames %ld\nok\n", runs, frames);
    return 0;
}
