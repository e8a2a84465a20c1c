/* fuzz_parse_streams.c -- the per-stream chains of heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams
 * (csrc/parse_streams.h, the host forms' pss_host) next to the host parser on chains of good, deferred and damaged
 * units, built with AddressSanitizer + UBSan by tests/test_parse_streams_core.py.
 *
 *   fuzz_parse_streams <seeds> <chains per stream>
 *
 * seeds: streams of { u32 chan_config, frames; per frame { u32 size; bytes } } (mono streams are parsed with PS).  Every
 * stream is first walked by the host parser, which registers its headers and leaves the states in front of each frame.
 * A chain is T = 1 .. 6 units from a random frame on: the stream's own frames in order, now and then another frame of
 * the stream (the seeds end in units the AAC half defers), a truncated, bit-flipped or random-tailed copy, or an empty
 * unit.  A streams call takes its units back to back behind one pointer, so the chain stands at the END of a heap block
 * of exactly its size (a byte read past its last unit is an ASan report; every third chain has one unit); for the host
 * parser every unit is copied to the end of a heap block of exactly ITS size, and a chain that read into its
 * neighbour would not come out with the host's bytes.  Both forms go through pss_host from the states in front of the
 * chain's first frame.  Rules, per chain and form:
 *   unit t < t0 (OK)   => the host parser takes it from the chain's state (HEAAC_PARSE_OK, or HEAAC_PARSE_NO_SBR for the HE
 *                         form) and coefficients, ics, tools, info, sbr and ps are the same bytes
 *   the host refuses   => the stream has stopped by then (the same rule read backwards); and where the host takes the
 *                         unit a stream stopped at, the reason is one of the deferred classes, never a refusal
 *   stopped at t0      => status, hold and taken say so for every unit, and both states are the host parser's after
 *                         unit t0 - 1 (t0 = 0: untouched)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "heaac_parse.h"
#include "parse_streams.h"

#define MAX_T 6
#define MAX_FRAMES 64

typedef struct { int chan_config, frames; int *size; uint8_t **au; HeaacAacStream ast[MAX_FRAMES]; HeaacSbrStream sst[MAX_FRAMES]; } Stream;

static uint32_t g_rng = 97531;
static uint32_t rnd(void) { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static long n_chains, n_taken, n_stopped, n_stopped_sbr, n_rewalk, n_host_refuses;
static HeaacSbrHeaderTable *g_tab;

static void fail(const char *what, const Stream *s, int he, int first, int t, int T)
{
    printf("FAIL: %s (chan_config %d, %s form, chain from frame %d, unit %d of %d)\n", what, s->chan_config, he ? "HE" : "AAC", first, t, T);
    exit(1);
}

static void make_cfg(HeaacAacConfig *cfg, const Stream *s)
{
    memset(cfg, 0, sizeof(*cfg));
    cfg->object_type = 2; cfg->sampling_index = 6; cfg->sample_rate = 24000; cfg->chan_config = s->chan_config;
    cfg->sbr = 1; cfg->ps = s->chan_config == 1; cfg->ext_object_type = 5; cfg->ext_sampling_index = 3; cfg->ext_sample_rate = 48000;
}

/* one unit through the host parser from (*ast, *sst), at the end of a heap block of exactly its size */
static int host_unit(const HeaacAacConfig *cfg, int he, int cc, HeaacAacStream *ast, HeaacSbrStream *sst, const uint8_t *bytes, int size,
                     float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools, HeaacSbrFrame *sbr, HeaacPsFrame *ps, HeaacAacFrameInfo *info)
{
    uint8_t *p = (uint8_t *)malloc(size ? (size_t)size : 1);
    if (!p) exit(2);
    memcpy(p, bytes, (size_t)size);
    const int r = he ? heaac_heaac_parse_frame_ex(cfg, ast, sst, g_tab, p, size, cc, coeffs, ics, tools, sbr, ps, info)
                     : heaac_aac_parse_frame_ex(cfg, ast, p, size, cc, coeffs, ics, tools, NULL, info);
    free(p);
    return r;
}

static void check(const Stream *s, int he, int first, const uint8_t *const *unit, const int *size, int T)
{
    static float ca[MAX_T * 2048], ch[2048];
    static HeaacToolsFrame ta[MAX_T], th;
    static HeaacSbrFrame ba[MAX_T], bh;
    static HeaacPsFrame pa[MAX_T], ph;
    HeaacIcs ia[MAX_T * 2], ih[2];
    HeaacAacFrameInfo fa[MAX_T], fh;
    int32_t status[MAX_T], why[MAX_T];
    uint8_t hold[MAX_T];
    uint32_t off[MAX_T + 1], taken = 99;
    HeaacAacConfig cfg;
    make_cfg(&cfg, s);
    const int cc = s->chan_config, with_ps = s->chan_config == 1;
    const HeaacParseTables *t = heaac_parse_tables();
    const HeaacSbrParseTables *stab = heaac_sbr_parse_tables();
    if (!t || !stab) exit(2);
    off[0] = 0;
    for (int k = 0; k < T; k++) off[k + 1] = off[k] + (uint32_t)size[k];
    uint8_t *p = (uint8_t *)malloc(off[T] ? off[T] : 1);
    if (!p) exit(2);
    for (int k = 0; k < T; k++) memcpy(p + off[k], unit[k], (size_t)size[k]);
    HeaacAacStream a = s->ast[first], h = s->ast[first];
    HeaacSbrStream sin = s->sst[first], sout, sh = s->sst[first];
    memset(&sout, 0xa5, sizeof(sout));
    memset(ca, 0xa5, sizeof(ca)); memset(ia, 0xa5, sizeof(ia)); memset(ta, 0xa5, sizeof(ta)); memset(fa, 0xa5, sizeof(fa));
    memset(ba, 0xa5, sizeof(ba)); memset(pa, 0xa5, sizeof(pa));
    memset(status, 0xa5, sizeof(status)); memset(why, 0xa5, sizeof(why)); memset(hold, 0xa5, sizeof(hold));
    const uint32_t n_hdr = (uint32_t)heaac_sbr_table_count(g_tab);       /* what the device holds: the headers so far */
    pss_host(&cfg, t, he ? stab : NULL, he, &a, he ? &sin : NULL, he ? &sout : NULL, p, off, 1, (uint32_t)T, cc, ca, ia, ta, fa,
             he ? heaac_sbr_table_data(g_tab) : NULL, n_hdr, he ? ba : NULL, he && with_ps ? pa : NULL, status, &taken, hold, why);
    free(p);
    n_chains++;
    if (taken > (uint32_t)T) fail("taken beyond T", s, he, first, 0, T);
    const int t0 = (int)taken;
    for (int k = 0; k < T; k++) {
        if (status[k] != (k < t0 ? HEAAC_PARSE_OK : HEAAC_PARSE_DEFERRED)) fail("status", s, he, first, k, T);
        if (hold[k] != (k >= t0)) fail("hold", s, he, first, k, T);
        if ((why[k] == 0) != (k < t0) || (k > t0 && why[k] != PSS_WHY_STOPPED)) fail("why", s, he, first, k, T);
    }
    for (int k = 0; k < t0; k++) {
        memset(ch, 0xa5, sizeof(ch)); memset(ih, 0xa5, sizeof(ih)); memset(&th, 0xa5, sizeof(th)); memset(&fh, 0xa5, sizeof(fh));
        memset(&bh, 0xa5, sizeof(bh)); memset(&ph, 0xa5, sizeof(ph));
        const int rh = host_unit(&cfg, he, cc, &h, &sh, unit[k], size[k], ch, ih, &th, &bh, with_ps ? &ph : NULL, &fh);
        if (rh != HEAAC_PARSE_OK && !(he && rh == HEAAC_PARSE_NO_SBR)) fail("unit taken, host parser does not take it", s, he, first, k, T);
        if (memcmp(ca + (size_t)k * cc * 1024, ch, sizeof(float) * (size_t)cc * 1024)) fail("coefficients differ", s, he, first, k, T);
        if (memcmp(ia + k * cc, ih, sizeof(HeaacIcs) * (size_t)cc)) fail("ics differs", s, he, first, k, T);
        if (memcmp(ta + k, &th, sizeof(th))) fail("tools differ", s, he, first, k, T);
        if (memcmp(fa + k, &fh, sizeof(fh))) fail("info differs", s, he, first, k, T);
        if (he && memcmp(ba + k, &bh, sizeof(bh))) fail("sbr record differs", s, he, first, k, T);
        if (he && with_ps && memcmp(pa + k, &ph, sizeof(ph))) fail("ps record differs", s, he, first, k, T);
        n_taken++;
    }
    /* both states as the host parser's after unit t0 - 1 */
    if (memcmp(&a, &h, sizeof(a))) fail("AAC state is not the one after the last unit taken", s, he, first, t0, T);
    if (he && memcmp(&sout, &sh, sizeof(sout))) fail("SBR state is not the one after the last unit taken", s, he, first, t0, T);
    if (t0 < T) {
        n_stopped++;
        const int by_sbr = why[t0] >= PSS_WHY_SBR;
        if (by_sbr) { n_stopped_sbr++; if (t0 >= 2) n_rewalk++; }
        const int rh = host_unit(&cfg, he, cc, &h, &sh, unit[t0], size[t0], ch, ih, &th, &bh, with_ps ? &ph : NULL, &fh);
        if (rh == HEAAC_PARSE_OK || (he && rh == HEAAC_PARSE_NO_SBR)) {
            const int r = why[t0];
            if (r != PC_WHY_PULSE && r != PC_WHY_ELEMENT && r != PSS_WHY_SBR * SC_WHY_HEADER && r != PSS_WHY_SBR * SC_WHY_MISPLACED)
                fail("stopped as refused, host parser takes the unit", s, he, first, t0, T);
        } else {
            n_host_refuses++;
        }
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    static Stream streams[64];
    int ns = 0;
    uint32_t hd[2];
    while (ns < 64 && fread(hd, 4, 2, f) == 2) {
        Stream *s = &streams[ns];
        s->chan_config = (int)hd[0]; s->frames = (int)hd[1];
        if (s->chan_config < 1 || s->chan_config > 2 || s->frames < 1 || s->frames > MAX_FRAMES) return 2;
        s->size = (int *)malloc(sizeof(int) * (size_t)s->frames);
        s->au = (uint8_t **)malloc(sizeof(uint8_t *) * (size_t)s->frames);
        if (!s->size || !s->au) return 2;
        for (int k = 0; k < s->frames; k++) {
            uint32_t size;
            if (fread(&size, 4, 1, f) != 1 || size < 1 || size > 8192) return 2;
            s->size[k] = (int)size;
            s->au[k] = (uint8_t *)malloc(size);
            if (!s->au[k] || fread(s->au[k], 1, size, f) != size) return 2;
        }
        ns++;
    }
    fclose(f);
    if (!ns) return 2;
    const long chains = atol(argv[2]);
    g_tab = heaac_sbr_table_create(65535);
    if (!g_tab) return 2;
    static uint8_t buf[MAX_T][8192];
    static float coeffs[2048];
    static HeaacToolsFrame tools;
    for (int k = 0; k < ns; k++) {
        Stream *s = &streams[k];
        HeaacAacConfig cfg;
        make_cfg(&cfg, s);
        HeaacAacStream ast;
        HeaacSbrStream sst;
        memset(&ast, 0, sizeof(ast));
        heaac_sbr_stream_init(&sst, 1);
        for (int t = 0; t < s->frames; t++) {                 /* the states in front of every frame, the headers registered */
            HeaacIcs ics[2];
            HeaacSbrFrame sbr;
            HeaacPsFrame ps;
            HeaacAacFrameInfo info;
            s->ast[t] = ast;
            s->sst[t] = sst;
            host_unit(&cfg, 1, s->chan_config, &ast, &sst, s->au[t], s->size[t], coeffs, ics, &tools, &sbr, s->chan_config == 1 ? &ps : NULL, &info);
        }
        for (long it = 0; it < chains; it++) {
            const int T = it % 3 == 0 ? 1 : 2 + (int)(rnd() % (MAX_T - 1));
            const int first = (int)(rnd() % (uint32_t)s->frames);
            const uint8_t *unit[MAX_T];
            int size[MAX_T];
            for (int u = 0; u < T; u++) {
                int from = first + u < s->frames ? first + u : (int)(rnd() % (uint32_t)s->frames);
                const uint32_t kind = rnd() % 20;
                if (kind == 0) from = (int)(rnd() % (uint32_t)s->frames);
                int n = s->size[from];
                memcpy(buf[u], s->au[from], (size_t)n);
                if (kind == 1) {
                    n = 1 + (int)(rnd() % (uint32_t)n);                                            /* truncated */
                } else if (kind == 2) {
                    for (int j = 1 + (int)(rnd() % 3); j > 0; j--) {                               /* bits flipped */
                        const uint32_t b = rnd() % (uint32_t)(n * 8);
                        buf[u][b >> 3] ^= (uint8_t)(0x80 >> (b & 7));
                    }
                } else if (kind == 3) {
                    for (int j = (int)(rnd() % (uint32_t)n); j < n; j++) buf[u][j] = (uint8_t)rnd();   /* a random tail */
                } else if (kind == 4) {
                    n = 0;                                                                         /* an empty unit */
                }
                unit[u] = buf[u];
                size[u] = n;
            }
            check(s, 1, first, unit, size, T);
            check(s, 0, first, unit, size, T);
        }
    }
    heaac_sbr_table_destroy(g_tab);
    printf("chains %ld: units taken %ld, streams stopped %ld of which by the SBR half %ld, second SBR walks over more than one unit %ld, "
           "host refuses the stopping unit %ld\n", n_chains, n_taken, n_stopped, n_stopped_sbr, n_rewalk, n_host_refuses);
    printf("ok\n");
    return 0;
}
