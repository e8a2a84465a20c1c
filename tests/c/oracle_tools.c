/* oracle_tools.c -- the oracle's spectral tools on the records of tests/edge_tools.py, as a process of its own so that
 * it can be built with AddressSanitizer + UBSan (tests/test_tools_reach.py links it with oracle/ *.c).  What the GPU
 * parity test compares against must be defined behaviour of the restated reference, not an out-of-range read.
 *
 * Input file: runs, one after the other, each
 *   int32 channels, n, steps, with_rng, with_pred
 *   int32 rng [n] (with_rng), HeaacPredictorState pred [n][channels][672] (with_pred)
 *   per step: float coeffs [n][channels][1024], HeaacToolsFrame [n]
 * Every stream chains its generator word and predictors through the steps.
 * Output: one line per run and "ok"; exit status 1 for a coefficient or predictor word that is not finite. */
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

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: oracle_tools records.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[5];
    int runs = 0;
    long frames = 0;
    while (fread(head, sizeof(head), 1, f) == 1) {
        const int channels = head[0], n = head[1], steps = head[2], with_rng = head[3], with_pred = head[4];
        if ((channels != 1 && channels != 2) || n < 1 || steps < 1) { fprintf(stderr, "bad run header\n"); return 2; }
        const size_t preds = (size_t)n * channels * HEAAC_MAX_PREDICTORS;
        int32_t *rng = with_rng ? take(f, (size_t)n * sizeof(*rng)) : NULL;
        HeaacPredictorState *pred = with_pred ? take(f, preds * sizeof(*pred)) : NULL;
        int finite = 1;
        for (int t = 0; t < steps; t++) {
            const size_t words = (size_t)n * channels * 1024;
            float *coeffs = take(f, words * sizeof(float));
            HeaacToolsFrame *tools = take(f, (size_t)n * sizeof(*tools));
            oracle_spectral_tools_batch(channels, coeffs, tools, rng, rng, pred, pred, (size_t)n);
            for (size_t i = 0; i < words; i++)
                if (!isfinite(coeffs[i])) finite = 0;
            for (size_t i = 0; pred && i < preds * 6; i++)
                if (!isfinite(((const float *)pred)[i])) finite = 0;
            free(coeffs); free(tools);
            frames += n;
        }
        printf("run %d: %d channels, %d streams x %d frames, rng %d pred %d, %s\n", runs, channels, n, steps, with_rng,
               with_pred, finite ? "finite" : "NOT FINITE");
        if (!finite) return 1;
        free(rng); free(pred);
        runs++;
    }
    fclose(f);
    printf("runs %d, frames %ld\nok\n", runs, frames);
    return 0;
}
