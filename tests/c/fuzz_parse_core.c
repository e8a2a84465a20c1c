/* fuzz_parse_core.c -- the access-unit walk of heaac_aac_parse_device (csrc/parse_core.h) next to the host parser on
 * damaged input, built with AddressSanitizer + UBSan by tests/test_parse_core.py.  Both go through the pc_* readers of
 * parse_core.h: the walk without a PcHost record (defer mode), the host parser with one (refuse mode).
 *
 *   fuzz_parse_core <seeds> <iterations>
 *
 * seeds: records of { u32 object_type, sampling_index, chan_config, size; bytes }.  Every seed, then `iterations`
 * mutations of them (truncated, bits flipped, spliced, random), each copied to the END of a heap block of exactly its
 * size -- one byte read past the unit is an ASan report -- and walked from a random stream state.  Rules:
 *   the walk says OK      => the host parser returns OK; state, coefficients, ics, tools and info are the same bytes
 *   the host refuses      => the walk defers
 *   the walk defers       => the state is untouched; and if the host parser takes the unit, the reason is pulse data
 *                            or an element outside the walk, never a refusal
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "heaac_parse.h"
#include "parse_core.h"

typedef struct { HeaacAacConfig cfg; int size; uint8_t *au; } Seed;

static uint32_t g_rng = 12345;
static uint32_t rnd(void) { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static long n_units, n_ok, n_def, n_def_host_ok, n_def_host_refused;

static void fail(const char *what, const Seed *s, int size)
{
    printf("FAIL: %s (aot %d si %d cc %d size %d)\n", what, s->cfg.object_type, s->cfg.sampling_index, s->cfg.chan_config, size);
    exit(1);
}

static void check(const Seed *s, const uint8_t *bytes, int size, const HeaacAacStream *st0, int cc)
{
    static float ca[2048], ch[2048];
    static HeaacToolsFrame ta, th;
    HeaacIcs ia[2], ih[2];
    HeaacAacFrameInfo fa, fh;
    HeaacAacStream a = *st0, h = *st0;
    const HeaacParseTables *t = heaac_parse_tables();
    uint8_t *p = (uint8_t *)malloc((size_t)size);
    if (!t || !p) fail("setup", s, size);
    memcpy(p, bytes, (size_t)size);
    memset(ca, 0xa5, sizeof(ca)); memset(ch, 0xa5, sizeof(ch));
    memset(ia, 0xa5, sizeof(ia)); memset(ih, 0xa5, sizeof(ih));
    memset(&fa, 0xa5, sizeof(fa)); memset(&fh, 0xa5, sizeof(fh));
    memset(&ta, 0, sizeof(ta)); memset(&th, 0xa5, sizeof(th));
    const int r = pc_walk(&s->cfg, t, &t->lut[0][0], &a, p, size, cc, ca, ia, &ta, &fa);
    const int rh = heaac_aac_parse_frame_ex(&s->cfg, &h, p, size, cc, ch, ih, &th, NULL, &fh);
    n_units++;
    if (r == 0) {
        n_ok++;
        if (rh != HEAAC_PARSE_OK) fail("walk OK, host parser refuses", s, size);
        if (memcmp(&a, &h, sizeof(a))) fail("state differs", s, size);
        if (memcmp(ca, ch, sizeof(ca))) fail("coefficients differ", s, size);
        if (memcmp(ia, ih, sizeof(ia))) fail("ics differs", s, size);
        if (memcmp(&ta, &th, sizeof(ta))) fail("tools differ", s, size);
        if (memcmp(&fa, &fh, sizeof(fa))) fail("info differs", s, size);
    } else {
        n_def++;
        if (memcmp(&a, st0, sizeof(a))) fail("deferred unit moved the state", s, size);
        if (rh == HEAAC_PARSE_OK) {
            n_def_host_ok++;
            if (r != PC_WHY_PULSE && r != PC_WHY_ELEMENT) fail("deferred as refused, host parser takes it", s, size);
        } else {
            n_def_host_refused++;
        }
    }
    free(p);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    static Seed seeds[8192];
    int ns = 0;
    uint32_t hd[4];
    while (ns < 8192 && fread(hd, 4, 4, f) == 4) {
        Seed *s = &seeds[ns];
        memset(&s->cfg, 0, sizeof(s->cfg));
        s->cfg.object_type = (int)hd[0]; s->cfg.sampling_index = (int)hd[1]; s->cfg.chan_config = (int)hd[2];
        s->cfg.sbr = -1; s->cfg.ps = (ns & 1) ? -1 : 0;
        s->size = (int)hd[3];
        s->au = (uint8_t *)malloc(hd[3] ? hd[3] : 1);
        if (!s->au || fread(s->au, 1, hd[3], f) != hd[3]) return 2;
        ns++;
    }
    fclose(f);
    if (!ns) return 2;
    HeaacAacStream zero;
    memset(&zero, 0, sizeof(zero));
    for (int k = 0; k < ns; k++)
        if (seeds[k].size > 0) check(&seeds[k], seeds[k].au, seeds[k].size, &zero, 2);
    const long iters = atol(argv[2]);
    static uint8_t buf[1 << 16];
    static const uint8_t ocs[8] = { 0, 1, 2, 4, 8, 12, 3, 9 };
    for (long it = 0; it < iters; it++) {
        const Seed *s = &seeds[rnd() % (uint32_t)ns];
        if (s->size <= 0 || s->size > (int)sizeof(buf) / 2) continue;
        int size = s->size;
        memcpy(buf, s->au, (size_t)size);
        switch (rnd() % 5) {
        case 0: size = 1 + (int)(rnd() % (uint32_t)size); break;                           /* truncated */
        case 1: for (int k = 1 + (int)(rnd() % 3); k > 0; k--) { const uint32_t b = rnd() % (uint32_t)(size * 8); buf[b >> 3] ^= (uint8_t)(0x80 >> (b & 7)); } break;
        case 2: {                                                                          /* spliced with another unit */
            const Seed *o = &seeds[rnd() % (uint32_t)ns];
            if (o->size > 0 && o->size <= (int)sizeof(buf) / 2) {
                const int cut = (int)(rnd() % (uint32_t)size), from = (int)(rnd() % (uint32_t)o->size);
                memcpy(buf + cut, o->au + from, (size_t)(o->size - from));
                size = cut + o->size - from;
            }
            break;
        }
        case 3: for (int k = (int)(rnd() % (uint32_t)size); k < size; k++) buf[k] = (uint8_t)rnd(); break;   /* random tail */
        default: break;                                                                    /* as it is, from another state */
        }
        HeaacAacStream st;
        memset(&st, 0, sizeof(st));
        st.window_sequence[0] = (uint8_t)(rnd() & 3); st.window_sequence[1] = (uint8_t)(rnd() & 3);
        st.use_kb_window[0] = (uint8_t)(rnd() & 1); st.use_kb_window[1] = (uint8_t)(rnd() & 1);
        st.mapped_tag = (uint8_t)(rnd() % 3);
        st.oc = ocs[rnd() & 7];
        check(s, buf, size, &st, s->cfg.chan_config == 1 && (rnd() & 1) ? 1 : 2);
    }
    printf("units %ld: core ok %ld, deferred %ld of which the host parser takes %ld, refuses %ld\n", n_units, n_ok, n_def,
           n_def_host_ok, n_def_host_refused);
    printf("ok\n");
    return 0;
}
