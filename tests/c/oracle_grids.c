/* oracle_grids.c -- the oracle's HE chains on the structural profiles' records, as a process of its own so that it can
 * be built with AddressSanitizer + UBSan (tests/test_grid_reach.py links it with oracle/ *.c).  What the GPU parity
 * test compares against must be defined behaviour of the restated reference, not an out-of-range read.
 *
 * Input file: runs, one after the other, each
 *   int32 cfg, flags, pcm_format, n, steps, n_hdr
 *   HeaacSbrHeader [n_hdr]
 *   per step: float coeffs [n][core][1024], HeaacIcs [n][core], HeaacSbrFrame [n], HeaacPsFrame [n] (HEAAC_CFG_HEV2 only)
 * Every stream starts from an all-zero state record and chains through the steps.
 * Output: one line per run and "ok"; exit status 1 for a call the oracle refuses or a state word that is not finite. */
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
    if (argc != 2) { fprintf(stderr, "usage: oracle_grids records.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[6];
    int runs = 0;
    long frames = 0;
    while (fread(head, sizeof(head), 1, f) == 1) {
        const int cfg = head[0], flags = head[1], fmt = head[2], n = head[3], steps = head[4], n_hdr = head[5];
        const int core = cfg == HEAAC_CFG_HEV1 ? 2 : 1, out_ch = cfg == HEAAC_CFG_HEV1_MONO ? 1 : 2;
        const int with_ps = cfg == HEAAC_CFG_HEV2;
        const size_t words = (size_t)core * HEAAC_ST_SAVED + (size_t)core * HEAAC_ST_SBR + (size_t)out_ch * HEAAC_ST_SYNTH +
                             (with_ps ? HEAAC_ST_PS : 0);
        if (n < 1 || steps < 1 || n_hdr < 1 || (cfg != HEAAC_CFG_HEV1 && cfg != HEAAC_CFG_HEV1_MONO && !with_ps)) {
            fprintf(stderr, "bad run header\n");
            return 2;
        }
        HeaacSbrHeader *hdr = take(f, (size_t)n_hdr * sizeof(*hdr));
        float *state = calloc((size_t)n * words, sizeof(float)), *next = calloc((size_t)n * words, sizeof(float));
        const size_t sample = fmt == HEAAC_PCM_F32_PLANAR ? sizeof(float) : sizeof(int16_t);
        void *pcm = malloc((size_t)n * out_ch * 2048 * sample);
        int finite = 1;
        for (int t = 0; t < steps; t++) {
            float *coeffs = take(f, (size_t)n * core * 1024 * sizeof(float));
            HeaacIcs *ics = take(f, (size_t)n * core * sizeof(*ics));
            HeaacSbrFrame *sbr = take(f, (size_t)n * sizeof(*sbr));
            HeaacPsFrame *ps = with_ps ? take(f, (size_t)n * sizeof(*ps)) : NULL;
            const int r = oracle_he_decode_batch_ex(cfg, flags, coeffs, ics, sbr, hdr, (size_t)n_hdr, ps, state, next, pcm, fmt,
                                                    (size_t)n);
            if (r) { fprintf(stderr, "run %d step %d: oracle_he_decode_batch_ex -> %d\n", runs, t, r); return 1; }
            float *swap = state; state = next; next = swap;
            for (size_t i = 0; i < (size_t)n * words; i++) {
                /* (the index words of the SBR record are integers stored in float words: small, so finite) */
                if (!isfinite(state[i])) finite = 0;
            }
            free(coeffs); free(ics); free(sbr); free(ps);
            frames += n;
        }
        printf("run %d: cfg %d flags %d format %d, %d streams x %d frames, state %s\n", runs, cfg, flags, fmt, n, steps,
               finite ? "finite" : "NOT FINITE");
        if (!finite) return 1;
        free(hdr); free(state); free(next); free(pcm);
        runs++;
    }
    fclose(f);
    printf("runs %d, frames %ld\nok\n", runs, frames);
    return 0;
}
