/* fuzz_sbr_core.c -- the SBR / PS payload walk of heaac_sbr_parse_device (csrc/sbr_core.h) next to the host parser on
 * damaged input, built with AddressSanitizer + UBSan by tests/test_sbr_core.py.
 *
 *   fuzz_sbr_core <seeds> <mutations per frame>
 *
 * seeds: streams of { u32 chan_config, frames; per frame { u32 size; bytes } } (mono streams are parsed with PS).  Every
 * stream is walked frame by frame on the host parser's states; each frame, and then `mutations` damaged copies of it
 * (truncated, bits flipped inside the payload or anywhere, a random tail), is copied to the END of a heap block of
 * exactly its size -- one byte read past the unit is an ASan report -- and goes through the walk and through
 * heaac_heaac_parse_frame_ex from the state the stream has in front of that frame.  Rules:
 *   the walk says OK      => the host returns HEAAC_PARSE_OK or HEAAC_PARSE_NO_SBR; state, sbr and ps are the same bytes
 *   the host returns else => the walk defers
 *   the walk defers       => if the host takes the unit, the reason is a header to register or a misplaced payload,
 *                            never a refusal (the state row of a deferred unit is the caller's to copy again)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "heaac_parse.h"
#include "sbr_core.h"

typedef struct { int chan_config, frames; int *size; uint8_t **au; } Stream;

static uint32_t g_rng = 4321;
static uint32_t rnd(void) { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static long n_units, n_ok, n_def, n_def_host_ok, n_def_host_refused, n_aac;
static HeaacSbrHeaderTable *g_tab;

static void fail(const char *what, const Stream *s, int frame, int size)
{
    printf("FAIL: %s (chan_config %d frame %d size %d)\n", what, s->chan_config, frame, size);
    exit(1);
}

/* One unit from the states (*ast, *sst).  carry: the host parser's states are written back.  Returns the host's info. */
static HeaacAacFrameInfo check(const Stream *s, int frame, const uint8_t *bytes, int size, HeaacAacStream *ast,
                               HeaacSbrStream *sst, int carry)
{
    static float coeffs[2048];
    static HeaacToolsFrame tools;
    HeaacIcs ics[2];
    HeaacAacFrameInfo info;
    HeaacAacConfig cfg;
    HeaacSbrFrame sbr_h, sbr_w;
    HeaacPsFrame ps_h, ps_w;
    const int with_ps = s->chan_config == 1;
    memset(&cfg, 0, sizeof(cfg));
    cfg.object_type = 2; cfg.sampling_index = 6; cfg.sample_rate = 24000; cfg.chan_config = s->chan_config;
    cfg.sbr = 1; cfg.ps = with_ps; cfg.ext_object_type = 5; cfg.ext_sampling_index = 3; cfg.ext_sample_rate = 48000;
    const HeaacSbrParseTables *t = heaac_sbr_parse_tables();
    uint8_t *p = (uint8_t *)malloc((size_t)size);
    if (!t || !p) fail("setup", s, frame, size);
    memcpy(p, bytes, (size_t)size);
    HeaacAacStream ah = *ast;
    HeaacSbrStream sh = *sst, sw = *sst;                 /* the walk works on a copy of the row: the out row */
    const uint32_t n_hdr = (uint32_t)heaac_sbr_table_count(g_tab);       /* what the device holds: the headers so far */
    memset(&sbr_h, 0xa5, sizeof(sbr_h)); memset(&ps_h, 0xa5, sizeof(ps_h));
    memset(&sbr_w, 0, sizeof(sbr_w)); memset(&ps_w, 0, sizeof(ps_w));   /* (the caller of the walk zeroes the records) */
    const int rh = heaac_heaac_parse_frame_ex(&cfg, &ah, &sh, g_tab, p, size, s->chan_config, coeffs, ics, &tools, &sbr_h,
                                              with_ps ? &ps_h : NULL, &info);
    n_units++;
    if (info.channels == 0) {
        n_aac++;                                         /* the AAC half refuses the unit: the walk is not reached */
    } else {
        const int r = sc_walk(&cfg, t, &sw, p, size, &info, heaac_sbr_table_data(g_tab), n_hdr, &sbr_w, with_ps ? &ps_w : NULL);
        const int host_takes = rh == HEAAC_PARSE_OK || rh == HEAAC_PARSE_NO_SBR;
        if (r == 0) {
            n_ok++;
            if (!host_takes) fail("walk OK, host parser does not take the unit", s, frame, size);
            if (memcmp(&sw, &sh, sizeof(sw))) fail("state differs", s, frame, size);
            if (memcmp(&sbr_w, &sbr_h, sizeof(sbr_w))) fail("sbr record differs", s, frame, size);
            if (with_ps && memcmp(&ps_w, &ps_h, sizeof(ps_w))) fail("ps record differs", s, frame, size);
        } else {
            n_def++;
            if (host_takes) {
                n_def_host_ok++;
                if (r != SC_WHY_HEADER && r != SC_WHY_MISPLACED) fail("deferred as refused, host parser takes it", s, frame, size);
            } else {
                n_def_host_refused++;
            }
        }
    }
    if (carry) { *ast = ah; *sst = sh; }
    free(p);
    return info;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    static Stream streams[256];
    int ns = 0;
    uint32_t hd[2];
    while (ns < 256 && fread(hd, 4, 2, f) == 2) {
        Stream *s = &streams[ns];
        s->chan_config = (int)hd[0]; s->frames = (int)hd[1];
        if (s->chan_config < 1 || s->chan_config > 2 || s->frames < 1 || s->frames > 64) return 2;
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
    const long iters = atol(argv[2]);
    g_tab = heaac_sbr_table_create(1024);
    if (!g_tab) return 2;
    static uint8_t buf[8192];
    for (int k = 0; k < ns; k++) {
        const Stream *s = &streams[k];
        HeaacAacStream ast;
        HeaacSbrStream sst;
        memset(&ast, 0, sizeof(ast));
        heaac_sbr_stream_init(&sst, 1);
        for (int t = 0; t < s->frames; t++) {
            HeaacAacStream a0 = ast;
            HeaacSbrStream s0 = sst;
            const HeaacAacFrameInfo info = check(s, t, s->au[t], s->size[t], &ast, &sst, 1);
            for (long it = 0; it < iters; it++) {
                int size = s->size[t];
                memcpy(buf, s->au[t], (size_t)size);
                const int first = info.sbr_payload_bit > 0 ? info.sbr_payload_bit : 0;
                const int span = info.sbr_payload_bit > 0 ? 8 * info.sbr_payload_bytes - 4 : 8 * size;
                switch (rnd() % 4) {
                case 0: size = 1 + (int)(rnd() % (uint32_t)size); break;                       /* truncated */
                case 1:                                                                        /* flips inside the payload */
                    for (int j = 1 + (int)(rnd() % 3); j > 0; j--) {
                        const uint32_t b = (uint32_t)first + rnd() % (uint32_t)span;
                        if (b < 8u * (uint32_t)size) buf[b >> 3] ^= (uint8_t)(0x80 >> (b & 7));
                    }
                    break;
                case 2:                                                                        /* flips anywhere */
                    for (int j = 1 + (int)(rnd() % 3); j > 0; j--) {
                        const uint32_t b = rnd() % (uint32_t)(size * 8);
                        buf[b >> 3] ^= (uint8_t)(0x80 >> (b & 7));
                    }
                    break;
                default:                                                                       /* a random tail */
                    for (int j = first / 8 + (int)(rnd() % (uint32_t)(size - first / 8)); j < size; j++) buf[j] = (uint8_t)rnd();
                    break;
                }
                HeaacAacStream a = a0;
                HeaacSbrStream ss = s0;
                check(s, t, buf, size, &a, &ss, 0);
            }
        }
    }
    heaac_sbr_table_destroy(g_tab);
    printf("units %ld: walk ok %ld, deferred %ld of which the host parser takes %ld, refuses %ld; AAC half refuses %ld\n", n_units,
           n_ok, n_def, n_def_host_ok, n_def_host_refused, n_aac);
    printf("ok\n");
    return 0;
}
