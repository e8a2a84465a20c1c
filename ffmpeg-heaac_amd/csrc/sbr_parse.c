/* sbr_parse.c -- the host's side of the SBR extension payload and its Parametric Stereo data
 * (include/heaac_parse.h, second slice).
 *
 * The payload syntax itself -- header fields, grid, dtdf, invf, envelopes, noise floors, harmonics, coupling, the PS
 * reader, the emit of the two records -- is written once, in sbr_core.h, for this file and for the device walk
 * (k_parse.hip); it is host-exact on every exit.  What stands here is what only the host does: the header table and a
 * header's application and registration, the misplaced-payload rule, the roll-back of a refused element, the private
 * PS cursor, the statuses and their order, the code-book table both callers walk (with the prefix table the host puts in
 * front of the walk), and the whole-unit entries with their threads.  The device defers every unit that needs one of
 * these.
 *
 * Own structure: the stream state is a plain record (HeaacSbrStream) the caller owns, one per stream; derived band
 * tables are never kept per stream -- a header that changes the tables is looked up in (or added to) a table shared by
 * the whole batch and the frame records carry its index, which is what heaac_he_decode_batch takes.
 *
 * The order of the payload follows the reference: ff_decode_sbr_extension (aacsbr.c:1044-1090), read_sbr_extension
 * (:900-926), read_sbr_data (:982-1020); for the readers see sbr_core.h.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "heaac_parse.h"
#include "sbr_iso_tables.h"
#include "parse_bits.h"
#include "sbr_core.h"
#include "validate.h"

enum { EXTENSION_ID_PS = 2 };

/* ------------------------------------------------------------------------------------------ */
/* code books: the ten SBR and the ten PS books of sbr_iso_tables.h (the order of the reference's enums,       */
/* aacsbr.c:45-56, aacps.c:50-61) as one flat table of tree nodes, built once with parse_bits.h's tree_build;    */
/* read here, and uploaded once per device context next to the tables of parse_core.h                           */
/* ------------------------------------------------------------------------------------------ */
static HeaacSbrParseTables g_st;
static uint16_t g_st_lut[HEAAC_ST_BOOKS << SC_LUT_BITS];  /* the host's prefix table in front of the walk (sc_tree) */
static int g_st_bad;                                   /* a code book did not fit (never with the shipped tables) */
static pthread_once_t g_st_once = PTHREAD_ONCE_INIT;

static void st_init(void)
{
    static Tree t;                                     /* 6 KB: not on the stack of whoever calls first */
    int total = 0;
    for (int k = 0; k < HEAAC_ST_BOOKS; k++) {
        const int ps = k >= 10, j = k % 10;
        const uint16_t *first = ps ? ps_huff_first : sbr_huff_first;
        g_st_bad |= tree_build(&t, (ps ? ps_huff_code : sbr_huff_code) + first[j], NULL,
                               (ps ? ps_huff_bits : sbr_huff_bits) + first[j], first[j + 1] - first[j]);
        if (total + t.count > HEAAC_ST_NODES) { g_st_bad = 1; return; }
        g_st.root[k] = (uint16_t)total;
        g_st.bias[k] = ps ? ps_huff_offset[j] : sbr_huff_lav[j];
        for (int i = 0; i < t.count; i++) {
            g_st.node[total + i][0] = t.n[i].child[0];
            g_st.node[total + i][1] = t.n[i].child[1];
        }
        total += t.count;
    }
    /* the prefix table: every code of up to SC_LUT_BITS bits, found by walking the nodes just laid down */
    for (int k = 0; k < HEAAC_ST_BOOKS; k++)
        for (int p = 0; p < 1 << SC_LUT_BITS; p++) {
            int at = g_st.root[k], c = 1;
            for (int d = 1; d <= SC_LUT_BITS && c > 0; d++) {
                c = g_st.node[at][(p >> (SC_LUT_BITS - d)) & 1];
                at = g_st.root[k] + c;
                if (c < 0) g_st_lut[(k << SC_LUT_BITS) + p] = (uint16_t)(d << 12 | (-c - 1));
            }
        }
}

/* The one host copy (NULL if a code book did not fit). */
const HeaacSbrParseTables *heaac_sbr_parse_tables(void)
{
    pthread_once(&g_st_once, st_init);
    return g_st_bad ? NULL : &g_st;
}

uint64_t heaac_sbr_tables_fingerprint(void)
{
    uint64_t h = 1469598103934665603ull;
#define MIX(arr) do { const uint8_t *p_ = (const uint8_t *)(arr); for (size_t i_ = 0; i_ < sizeof(arr); i_++) { h ^= p_[i_]; h *= 1099511628211ull; } } while (0)
    MIX(sbr_huff_first); MIX(sbr_huff_code); MIX(sbr_huff_bits); MIX(sbr_huff_lav);
    MIX(ps_huff_first); MIX(ps_huff_code); MIX(ps_huff_bits); MIX(ps_huff_offset);
#undef MIX
    return h;
}

/* ------------------------------------------------------------------------------------------ */
/* header table                                                                                  */
/* ------------------------------------------------------------------------------------------ */
typedef struct { int32_t v[13]; } HdrKey;            /* SBR rate + the 12 header fields */

struct HeaacSbrHeaderTable {
    HeaacSbrHeader *h;
    HdrKey *key;
    size_t cap;
    volatile size_t n;
    pthread_mutex_t lock;
};

HeaacSbrHeaderTable *heaac_sbr_table_create(size_t capacity)
{
    if (capacity < 1 || capacity > 65535) return NULL;
    HeaacSbrHeaderTable *t = (HeaacSbrHeaderTable *)calloc(1, sizeof(*t));
    if (!t) return NULL;
    t->h = (HeaacSbrHeader *)calloc(capacity, sizeof(HeaacSbrHeader));
    t->key = (HdrKey *)calloc(capacity, sizeof(HdrKey));
    if (!t->h || !t->key) { free(t->h); free(t->key); free(t); return NULL; }
    t->cap = capacity;
    pthread_mutex_init(&t->lock, NULL);
    /* entry 0: no header yet */
    t->h[0].kx = 32;
    memset(t->h[0].map_hi, 0xff, 6 * 64);
    for (int i = 0; i < 13; i++) t->key[0].v[i] = -1;
    t->n = 1;
    return t;
}

void heaac_sbr_table_destroy(HeaacSbrHeaderTable *t)
{
    if (!t) return;
    pthread_mutex_destroy(&t->lock);
    free(t->h); free(t->key); free(t);
}

size_t heaac_sbr_table_count(const HeaacSbrHeaderTable *t) { return t ? t->n : 0; }
const HeaacSbrHeader *heaac_sbr_table_data(const HeaacSbrHeaderTable *t) { return t ? t->h : NULL; }

/* index of the header built from `k`, -1: the tables cannot be built (sbr_reset fails), -2: table full */
static int table_find_or_add(HeaacSbrHeaderTable *t, const HdrKey *k)
{
    int idx = -1;
    pthread_mutex_lock(&t->lock);
    for (size_t i = 1; i < t->n; i++)
        if (!memcmp(&t->key[i], k, sizeof(*k))) { idx = (int)i; break; }
    if (idx < 0) {
        if (t->n >= t->cap) {
            idx = -2;
        } else {
            HeaacSbrHeader h;
            const int32_t *v = k->v;
            /* a header the reference builds but whose tables the decode kernels cannot take (no limiter band
             * left over a dropped patch: the reference then reads gains of earlier frames) counts as not built */
            if (heaac_sbr_make_header(&h, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]) == 0 &&
                heaac_check_sbr_header(&h) == HEAAC_BAD_NONE) {
                t->h[t->n] = h;
                t->key[t->n] = *k;
                __sync_synchronize();                 /* the entry is complete before it becomes visible */
                idx = (int)t->n;
                t->n = t->n + 1;
            }
        }
    }
    pthread_mutex_unlock(&t->lock);
    return idx;
}

static void make_key(HdrKey *k, const HeaacSbrStream *s, int sbr_rate)
{
    k->v[0] = sbr_rate;
    k->v[1] = s->bs_start_freq;  k->v[2] = s->bs_stop_freq;   k->v[3] = s->bs_xover_band;
    k->v[4] = s->bs_freq_scale;  k->v[5] = s->bs_alter_scale; k->v[6] = s->bs_noise_bands;
    k->v[7] = s->bs_limiter_bands; k->v[8] = s->bs_limiter_gains;
    k->v[9] = s->bs_interpol_freq; k->v[10] = s->bs_smoothing_mode; k->v[11] = s->bs_amp_res_header;
    k->v[12] = 0;
}

/* ------------------------------------------------------------------------------------------ */
/* stream state                                                                                  */
/* ------------------------------------------------------------------------------------------ */
void heaac_sbr_stream_init(HeaacSbrStream *st, size_t n)
{
    memset(st, 0, n * sizeof(*st));
    for (size_t i = 0; i < n; i++) {
        st[i].kx[0] = st[i].kx[1] = 32;               /* ff_aac_sbr_ctx_init, aacsbr.c:130-131 */
        st[i].data[0].e_a[1] = st[i].data[1].e_a[1] = -1;
    }
}

size_t heaac_sbr_stream_bytes(void) { return sizeof(HeaacSbrStream); }

/* ------------------------------------------------------------------------------------------ */
/* payload                                                                                       */
/* ------------------------------------------------------------------------------------------ */
/* A header is always applied (read_sbr_header stores what it reads), whatever it changes. */
static void apply_header(HeaacSbrStream *s, const ScHeader *hd)
{
    s->start = 1;
    s->bs_amp_res_header = hd->amp_res;
    s->bs_start_freq = hd->start_freq;   s->bs_stop_freq = hd->stop_freq;       s->bs_xover_band = hd->xover_band;
    s->bs_freq_scale = hd->freq_scale;   s->bs_alter_scale = hd->alter_scale;   s->bs_noise_bands = hd->noise_bands;
    s->bs_limiter_bands = hd->limiter_bands; s->bs_limiter_gains = hd->limiter_gains;
    s->bs_interpol_freq = hd->interpol_freq; s->bs_smoothing_mode = hd->smoothing_mode;
}

/* Parametric Stereo through a private cursor: the SBR reader's own moves over the frame only when it is good.  On an
 * error PS is switched off (ps->start = 0; the rest of *ps is as sc_ps left it), the rest of the extension is skipped
 * and *status says which error it was.  Returns the bits the SBR reader steps over. */
static int read_ps(const HeaacSbrParseTables *t, PcBits *host, HeaacPsState *ps, int bits_left_in_ext, int *status)
{
    PcBits own = *host;
    const int used = sc_ps(t, g_st_lut, &own, ps, bits_left_in_ext);
    if (used >= 0) {
        *host = own;
        *status = HEAAC_PARSE_OK;
        return used;
    }
    *status = used == SC_PS_ERR_OVERREAD ? HEAAC_PARSE_ERR_OVERREAD : HEAAC_PARSE_ERR_DATA;
    ps->start = 0;
    host->pos += bits_left_in_ext;
    return bits_left_in_ext;
}

void heaac_sbr_no_payload(HeaacSbrStream *st, int channels, HeaacSbrFrame *sbr, HeaacPsFrame *ps)
{
    st->kx[0] = st->kx[1];
    st->m[0] = st->m[1];
    memset(sbr, 0, sizeof(*sbr));
    sc_emit_sbr(st, NULL, channels, 0, 0, sbr);
    if (ps) {
        memset(ps, 0, sizeof(*ps));
        sc_emit_ps(&st->ps, ps);
    }
}

/* ff_decode_sbr_extension (aacsbr.c:1044-1090) + read_sbr_data (:982-1020) */
int heaac_sbr_parse_payload(HeaacSbrStream *st, HeaacSbrHeaderTable *tab, int sample_rate,
                            const uint8_t *au, int size, int bit, int cnt, int crc,
                            int channels, int allow_ps,
                            HeaacSbrFrame *sbr, HeaacPsFrame *ps, HeaacSbrParseInfo *info)
{
    if (!st || !tab || !au || !sbr || size < 0 || bit < 0 || bit > 8 * size || cnt < 0 ||
        (channels != 1 && channels != 2) || (allow_ps & ~(HEAAC_SBR_ALLOW_PS | HEAAC_SBR_MISPLACED)) ||
        ((allow_ps & HEAAC_SBR_ALLOW_PS) && !ps))
        return HEAAC_PARSE_ERR_ARG;
    const int misplaced = allow_ps & HEAAC_SBR_MISPLACED;
    allow_ps &= HEAAC_SBR_ALLOW_PS;
    const HeaacSbrParseTables *t = heaac_sbr_parse_tables();
    if (!t) return HEAAC_PARSE_ERR_ARG;

    PcBits gb, *b = &gb;
    pc_init(b, au, size);
    b->pos = bit;
    int ret = HEAAC_PARSE_OK;
    HeaacSbrParseInfo fi = { 0, 0, 0, HEAAC_PARSE_OK };

    st->reset = 0;
    if (crc) pc_bits(b, 10);                           /* bs_sbr_crc_bits: not checked by the reference either */
    st->kx[0] = st->kx[1];
    st->m[0]  = st->m[1];

    if (pc_bit1(b)) {                                  /* bs_header_flag */
        ScHeader hd;
        fi.header = 1;
        sc_read_header(b, &hd);
        const int touched = sc_header_touches(st, &hd);
        st->reset = (uint8_t)sc_header_resets(st, &hd);
        apply_header(st, &hd);
        if (st->reset || (touched && st->hdr)) {
            HdrKey k;
            make_key(&k, st, 2 * sample_rate);
            const int idx = table_find_or_add(tab, &k);
            if (idx > 0) {
                st->hdr = (uint32_t)idx;
                st->have_spectrum = 1;
                st->kx[1] = tab->h[idx].kx;
                st->m[1]  = tab->h[idx].m;
            } else {                                   /* sbr_reset failed (:1029-1033) or no room */
                st->start = 0;
                st->have_spectrum = 0;
                ret = idx == -2 ? HEAAC_PARSE_ERR_ARG : HEAAC_PARSE_ERR_DATA;
            }
        }
    }

    if (st->start && misplaced) {
        /* read_sbr_data with the type of a fill / data stream / program config element or an LFE (aacsbr.c:996-1000):
         * "Invalid bitstream - cannot apply SBR to element type %d" */
        st->start = 0;
        ret = HEAAC_PARSE_ERR_DATA;
    } else if (st->start) {
        const HeaacSbrHeader *h = &tab->h[st->hdr];
        const HeaacSbrChanState keep0 = st->data[0], keep1 = st->data[1];
        const uint8_t keep_coupling = st->bs_coupling;
        if (sc_element(t, g_st_lut, st, h, b, channels)) {       /* refused: the channels are as they were before it */
            st->data[0] = keep0; st->data[1] = keep1; st->bs_coupling = keep_coupling;
            st->start = 0;
            ret = HEAAC_PARSE_ERR_DATA;
        } else if (pc_bit1(b)) {                       /* bs_extended_data */
            int left = (int)pc_bits(b, 4);
            if (left == 15) left += (int)pc_bits(b, 8);
            left <<= 3;
            while (left > 7) {
                left -= 2;
                const int id = (int)pc_bits(b, 2);
                if (id == EXTENSION_ID_PS && allow_ps) {
                    fi.ps_present = 1;
                    left -= read_ps(t, b, &st->ps, left, &fi.ps_status);
                } else {                               /* PS signalled absent, or a reserved extension */
                    b->pos += left;
                    left = 0;
                }
            }
            if (left > 0) b->pos += left;
        }
    }
    fi.sbr_bits = b->pos - bit;
    if (b->over && ret == HEAAC_PARSE_OK) ret = HEAAC_PARSE_ERR_OVERREAD;

    memset(sbr, 0, sizeof(*sbr));
    sc_emit_sbr(st, &tab->h[st->hdr], channels, st->start, st->reset, sbr);
    if (ps) {
        memset(ps, 0, sizeof(*ps));
        sc_emit_ps(&st->ps, ps);
    }
    if (info) *info = fi;
    if (ret == HEAAC_PARSE_OK && fi.ps_status) ret = fi.ps_status;
    return ret;
}

/* ------------------------------------------------------------------------------------------ */
/* whole access units                                                                            */
/* ------------------------------------------------------------------------------------------ */
int heaac_heaac_parse_frame(const HeaacAacConfig *cfg, HeaacAacStream *st, HeaacSbrStream *sst,
                            HeaacSbrHeaderTable *tab, const uint8_t *au, int size,
                            float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                            HeaacSbrFrame *sbr, HeaacPsFrame *ps, HeaacAacFrameInfo *info)
{
    return heaac_heaac_parse_frame_ex(cfg, st, sst, tab, au, size, 2, coeffs, ics, tools, sbr, ps, info);
}

int heaac_heaac_parse_frame_ex(const HeaacAacConfig *cfg, HeaacAacStream *st, HeaacSbrStream *sst,
                               HeaacSbrHeaderTable *tab, const uint8_t *au, int size, int coeff_channels,
                               float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                               HeaacSbrFrame *sbr, HeaacPsFrame *ps, HeaacAacFrameInfo *info)
{
    HeaacAacFrameInfo fi;
    memset(&fi, 0, sizeof(fi));
    if (info) *info = fi;
    if (!cfg || !sst || !tab || !sbr) return HEAAC_PARSE_ERR_ARG;
    const int r = heaac_aac_parse_frame_ex(cfg, st, au, size, coeff_channels, coeffs, ics, tools, NULL, &fi);
    if (info) *info = fi;                              /* refused: channels = 0 and the HEAAC_REFUSED_* flags */
    if (r) return r;
    const int allow_ps = (cfg->ps != 0 && fi.channels == 1 && ps != NULL ? HEAAC_SBR_ALLOW_PS : 0) |
                         (fi.sbr_misplaced ? HEAAC_SBR_MISPLACED : 0);
    if (fi.sbr_payload_bit < 0 || cfg->sbr == 0) {
        heaac_sbr_no_payload(sst, fi.channels, sbr, ps);
        return HEAAC_PARSE_NO_SBR;
    }
    return heaac_sbr_parse_payload(sst, tab, cfg->sample_rate, au, size, fi.sbr_payload_bit, fi.sbr_payload_bytes,
                                   fi.sbr_crc, fi.channels, allow_ps, sbr, ps, NULL);
}

typedef struct {
    const HeaacAacConfig *cfg; HeaacAacStream *st; HeaacSbrStream *sst; HeaacSbrHeaderTable *tab;
    const uint8_t *const *au; const int *size;
    float *coeffs; HeaacIcs *ics; HeaacToolsFrame *tools; HeaacSbrFrame *sbr; HeaacPsFrame *ps;
    HeaacAacFrameInfo *info; int *status;
    size_t lo, hi; int failed;
} Job;

static void *job_run(void *p)
{
    Job *j = (Job *)p;
    for (size_t i = j->lo; i < j->hi; i++) {
        const int r = heaac_heaac_parse_frame(j->cfg, &j->st[i], &j->sst[i], j->tab, j->au[i], j->size[i],
                                              j->coeffs + i * 2048, j->ics + 2 * i, &j->tools[i],
                                              &j->sbr[i], j->ps ? &j->ps[i] : NULL, j->info ? &j->info[i] : NULL);
        if (j->status) j->status[i] = r;
        j->failed += r < 0;
    }
    return NULL;
}

int heaac_heaac_parse_batch(const HeaacAacConfig *cfg, HeaacAacStream *st, HeaacSbrStream *sst,
                            HeaacSbrHeaderTable *tab,
                            const uint8_t *const *au, const int *size, size_t n,
                            float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                            HeaacSbrFrame *sbr, HeaacPsFrame *ps,
                            HeaacAacFrameInfo *info, int *status, int threads)
{
    if (!cfg || !st || !sst || !tab || !au || !size || !coeffs || !ics || !tools || !sbr) return HEAAC_PARSE_ERR_ARG;
    if (threads <= 0) threads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (threads < 1) threads = 1;
    if ((size_t)threads > n) threads = n ? (int)n : 1;
    if (threads > 256) threads = 256;
    Job job[256];
    pthread_t tid[256];
    int started[256];
    for (int t = 0; t < threads; t++) {
        job[t] = (Job){ cfg, st, sst, tab, au, size, coeffs, ics, tools, sbr, ps, info, status,
                        n * (size_t)t / (size_t)threads, n * (size_t)(t + 1) / (size_t)threads, 0 };
        started[t] = t > 0 && pthread_create(&tid[t], NULL, job_run, &job[t]) == 0;
    }
    job_run(&job[0]);
    int failed = job[0].failed;
    for (int t = 1; t < threads; t++) {
        if (started[t]) pthread_join(tid[t], NULL);
        else job_run(&job[t]);
        failed += job[t].failed;
    }
    return failed;
}
