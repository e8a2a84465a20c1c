/* pipeline_pack.c -- the two plain-C steps of a device-parse tick (csrc/pipeline_pack.h) under ASan / UBSan, stand-alone:
 * every unit sits at the very end of a heap block of exactly its size, so a read one byte past a unit is caught; the
 * packed buffer has exactly the tick's bytes, so a write past it is caught too.  Empty units carry NULL and must
 * not be looked at.  The stop list is held against a count made here.
 * Prints what it saw; exit status 0 = every check passed (tests/test_pipeline_device_parse.py runs it). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pipeline_pack.h"

static uint32_t rnd_state = 12345;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "pipeline_pack.c:%d: %s\n", __LINE__, #c); return 1; } } while (0)

static int pack_round(size_t n, int empties)
{
    uint8_t **au = (uint8_t **)calloc(n ? n : 1, sizeof(*au));
    int *size = (int *)calloc(n ? n : 1, sizeof(*size));
    uint32_t *off = (uint32_t *)malloc((n + 1) * sizeof(*off));
    CHECK(au && size && off);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t r = rnd();
        if (empties == 2 || (empties && r % 4 == 0)) { size[i] = r % 8 == 0 ? -(int)(r % 1000) : 0; au[i] = NULL; continue; }
        size[i] = 1 + (int)(r % 700);
        au[i] = (uint8_t *)malloc((size_t)size[i]);          /* the unit ends where its block ends */
        CHECK(au[i]);
        for (int k = 0; k < size[i]; k++) au[i][k] = (uint8_t)(i * 31 + (size_t)k * 7);
        total += (size_t)size[i];
    }
    CHECK(heaac_pack_offsets(size, n, off) == 0);
    CHECK(off[0] == 0 && off[n] == total);
    uint8_t *bytes = (uint8_t *)malloc(total ? total : 1);   /* exactly the tick's bytes */
    CHECK(bytes);
    /* in slices, as the pool does it */
    const size_t W = 3;
    for (size_t w = 0; w < W; w++)
        heaac_pack_bytes((const uint8_t *const *)au, size, off, n * w / W, n * (w + 1) / W, bytes);
    for (size_t i = 0; i < n; i++) {
        const size_t len = size[i] > 0 ? (size_t)size[i] : 0;
        CHECK(off[i + 1] - off[i] == len);
        for (size_t k = 0; k < len; k++) CHECK(bytes[off[i] + k] == (uint8_t)(i * 31 + k * 7));
        free(au[i]);
    }
    free(bytes); free(off); free(size); free(au);
    return 0;
}

static int refusal(void)
{
    /* three units of 2^31 - 1 bytes: from the sizes alone */
    int size[3] = { 0x7fffffff, 0x7fffffff, 0x7fffffff };
    uint32_t off[4];
    CHECK(heaac_pack_offsets(size, 3, off) == -1);
    size[2] = 1;                                            /* 2^32 - 1: the largest tick */
    CHECK(heaac_pack_offsets(size, 3, off) == 0 && off[3] == 0xffffffffu && off[2] == 0xfffffffeu);
    size[2] = 2;
    CHECK(heaac_pack_offsets(size, 3, off) == -1);
    return 0;
}

static int stops_round(size_t n, uint32_t T)
{
    uint32_t *taken = (uint32_t *)malloc((n ? n : 1) * sizeof(*taken));
    uint32_t *list = (uint32_t *)malloc((n ? n : 1) * sizeof(*list));        /* exactly [n] */
    uint32_t *base = (uint32_t *)malloc((n + 1) * sizeof(*base));            /* exactly [n + 1] */
    CHECK(taken && list && base);
    size_t want_m = 0, want_units = 0;
    for (size_t s = 0; s < n; s++) {
        taken[s] = rnd() % 3 == 0 ? rnd() % (T + 1) : T;
        if (n < 4) taken[s] = (uint32_t)s % (T + 1);                         /* small cases: every stream stops early */
        if (taken[s] < T) { want_m++; want_units += T - taken[s]; }
    }
    const size_t m = heaac_stop_list(taken, n, T, list, base);
    CHECK(m == want_m && base[m] == want_units);
    for (size_t j = 0; j < m; j++) {
        CHECK(list[j] < n && taken[list[j]] < T);
        CHECK(j == 0 || list[j] > list[j - 1]);
        CHECK(base[j + 1] - base[j] == T - taken[list[j]]);
    }
    free(base); free(list); free(taken);
    return 0;
}

int main(void)
{
    int rounds = 0;
    for (size_t n = 0; n < 40; n++)
        for (int e = 0; e < 2; e++, rounds++)
            if (pack_round(n, e)) return 1;
    if (pack_round(5000, 1)) return 1;
    if (pack_round(9, 2)) return 1;                         /* a tick of nothing but empty units */
    if (refusal()) return 1;
    for (size_t n = 0; n < 70; n++)
        for (uint32_t T = 1; T <= 5; T++, rounds++)
            if (stops_round(n, T)) return 1;
    printf("pipeline_pack: %d rounds ok\n", rounds + 3);
    return 0;
}
