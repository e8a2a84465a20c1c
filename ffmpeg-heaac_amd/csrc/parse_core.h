/* parse_core.h -- the access-unit walk of heaac_aac_parse_device (include/heaac_parse.h), written once for the host
 * and the device.
 *
 * A second, independent writing of what aac_parse.c's frame_walk does for the common case: one SCE or one CPE per
 * unit, AAC-LC / AAC-Main, data stream and fill elements skipped, an ADTS header in front.  It takes its tables, the
 * unit and the stream state by pointer and performs no I/O; k_parse.hip instantiates it one lane per unit, and for the
 * host (heaac_debug_aac_parse_core, include/heaac_debug.h), where it is tested, fuzzed and debugged.
 *
 * It never decides a refusal.  Wherever aac_parse.c would return anything but HEAAC_PARSE_OK the walk gives the unit
 * up (a PC_WHY_* reason, status HEAAC_PARSE_DEFERRED) and the caller hands it to the host parser, which holds the
 * HEAAC_REFUSED_* rules; so does a unit with pulse data (pulse_add goes through libm's cbrtf on an arbitrary float)
 * and one with a CCE, PCE, LFE or a second SCE / CPE.  The stream state is worked on in a copy and committed on OK
 * only.  The records of a unit that is given up are unspecified.
 *
 * The caller zeroes the unit's HeaacToolsFrame ahead of the walk (the host parser's memset).
 *
 * Termination: every loop is bounded by the unit's bits (each pass consumes at least one, and a read past the end
 * ends the walk at the next check) or by a constant.
 */
#ifndef HEAAC_PARSE_CORE_H
#define HEAAC_PARSE_CORE_H

#include <stdint.h>
#include <string.h>
#include "heaac_parse.h"

#if defined(__HIPCC__)
#define PC_FN static __host__ __device__ inline
#else
#define PC_FN static inline
#endif

#define HEAAC_PT_BOOKS 12             /* 0: scalefactors, 1..11: spectral books */
#define HEAAC_PT_LUT 1024             /* ten-bit prefix table (TREE_LUT_BITS of parse_bits.h) */
#define HEAAC_PT_NODES 580            /* TREE_MAX_NODES of parse_bits.h */

typedef struct HeaacParseTables {
    uint32_t lut[HEAAC_PT_BOOKS][HEAAC_PT_LUT];
    int16_t  node[HEAAC_PT_BOOKS][HEAAC_PT_NODES][2];
    float    pow2sf[428];
    float    mag[16];
    float    esc[8192];
    float    tns_map[4][16];
    uint16_t swb_first_1024[13], swb_first_128[13];
    uint16_t swb_offset_1024[594], swb_offset_128[196];
    uint8_t  num_swb_1024[13], num_swb_128[13], pred_sfb_max[13], tns_max_bands_1024[13], tns_max_bands_128[13];
} HeaacParseTables;

#ifdef __cplusplus
extern "C" {
#endif
const HeaacParseTables *heaac_parse_tables(void);     /* parse_tables.c */
#ifdef __cplusplus
}
#endif

/* why a unit was given up (heaac_debug_aac_parse_core reports it; the status of the call is HEAAC_PARSE_DEFERRED) */
#define PC_WHY_PULSE    1             /* pulse data */
#define PC_WHY_ELEMENT  2             /* a CCE, PCE or LFE, or a second SCE / CPE */
#define PC_WHY_REFUSED  4             /* a check of the host parser that the unit does not pass */

#define PC_OC_LOCKED 1u               /* HeaacAacStream.oc, as aac_parse.c names the bits */
#define PC_OC_NONE   2u
#define PC_OC_PS     4u
#define PC_OC_TWO    8u

/* ---- bit reader: MSB first, zeros past the end and `over` set, as parse_bits.h; the unit is read eight bytes at a
 * time into a window, and no byte outside [buf, buf + size_bytes) is ever touched ---- */
typedef struct PcBits {
    const uint8_t *buf;
    int size_bytes, size_bits, pos, over;
    uint64_t win;
    int wpos;                         /* bit position of the window's first bit; -1: empty */
} PcBits;

PC_FN void pc_init(PcBits *b, const uint8_t *buf, int bytes)
{
    b->buf = buf; b->size_bytes = bytes; b->size_bits = bytes * 8; b->pos = 0; b->over = 0; b->win = 0; b->wpos = -1;
}
PC_FN uint32_t pc_peek32(PcBits *b)
{
    if (b->wpos < 0 || b->pos < b->wpos || b->pos > b->wpos + 32) {
        const int byte = b->pos >> 3;
        uint64_t v = 0;
        if (byte <= b->size_bytes - 8) {
            memcpy(&v, b->buf + byte, 8);
            v = __builtin_bswap64(v);
        } else {
            for (int i = 0; i < 8; i++) {
                v <<= 8;
                if (byte < b->size_bytes - i) v |= b->buf[byte + i];
            }
        }
        b->win = v;
        b->wpos = byte << 3;
    }
    return (uint32_t)((b->win << (b->pos - b->wpos)) >> 32);
}
PC_FN void pc_skip(PcBits *b, int n)
{
    b->pos += n;
    if (b->pos > b->size_bits) b->over = 1;
}
PC_FN unsigned pc_bits(PcBits *b, int n)             /* n <= 25 */
{
    if (n <= 0) return 0;
    const unsigned v = pc_peek32(b) >> (32 - n);
    pc_skip(b, n);
    return v;
}
PC_FN unsigned pc_bit1(PcBits *b) { return pc_bits(b, 1); }
PC_FN int pc_left(const PcBits *b) { return b->size_bits - b->pos; }

/* tree_read of parse_bits.h: -1 for a prefix that is no code of the book.  `lut` = the twelve prefix tables
 * ([HEAAC_PT_BOOKS][HEAAC_PT_LUT], on the device a copy in LDS), the nodes beyond ten bits come from t->node. */
PC_FN int pc_tree(const HeaacParseTables *t, const uint32_t *lut, int book, PcBits *b)
{
    const uint32_t w = pc_peek32(b);
    const uint32_t e = lut[book * HEAAC_PT_LUT + (w >> 22)];
    const unsigned len = e >> 16;
    if (len == 0xff) return -1;
    if (len) { pc_skip(b, (int)len); return (int)(e & 0xffff); }
    int at = (int)e;
    for (int d = 10; d < 32; d++) {
        const int c = t->node[book][at][(w >> (31 - d)) & 1];
        if (c < 0) { pc_skip(b, d + 1); return -c - 1; }
        if (c == 0) return -1;
        at = c;
    }
    return -1;
}

/* the window history of one channel packed as HeaacIcs lies in memory: window_sequence[0], [1], use_kb_window[0], [1] */
#define PC_WS0(w) ((w) & 0xffu)
#define PC_KB0(w) (((w) >> 16) & 0xffu)

#if defined(__HIP_DEVICE_COMPILE__)
#define PC_ST4(p, a, b_, c, d) (*(float4 *)(p) = make_float4((a), (b_), (c), (d)))
#define PC_ST2(p, a, b_) (*(float2 *)(p) = make_float2((a), (b_)))
#else
#define PC_ST4(p, a, b_, c, d) ((p)[0] = (a), (p)[1] = (b_), (p)[2] = (c), (p)[3] = (d))
#define PC_ST2(p, a, b_) ((p)[0] = (a), (p)[1] = (b_))
#endif

PC_FN void pc_zero(float *p, int n)                   /* n a multiple of 4, p 16-byte aligned (band offsets are) */
{
    for (int k = 0; k < n; k += 4) PC_ST4(p + k, 0.0f, 0.0f, 0.0f, 0.0f);
}

/* decode_ics_info + decode_prediction; *win: the channel's history moves on to this unit's */
PC_FN int pc_ics_info(const HeaacAacConfig *cfg, const HeaacParseTables *t, PcBits *b, HeaacToolsChannel *ch, uint32_t *win)
{
    const int si = cfg->sampling_index;
    HeaacToolsIcs *ics = &ch->ics;
    HeaacPrediction *pred = &ch->pred;
    if (pc_bit1(b)) return PC_WHY_REFUSED;
    const unsigned ws = pc_bits(b, 2), kb = pc_bit1(b);
    *win = ws | (PC_WS0(*win) << 8) | (kb << 16) | (PC_KB0(*win) << 24);
    int num_groups = 1;
    ics->group_len[0] = 1;
    pred->pred_sfb_max = t->pred_sfb_max[si];
    const uint16_t *src;
    if (ws == 2) {                                    /* EIGHT_SHORT_SEQUENCE */
        ics->max_sfb = (uint8_t)pc_bits(b, 4);
        const unsigned grouping = pc_bits(b, 7);
        int len = 1;
        for (int i = 0; i < 7; i++) {
            if ((grouping >> (6 - i)) & 1) {
                len++;
            } else {
                ics->group_len[num_groups - 1] = (uint8_t)len;
                num_groups++;
                len = 1;
            }
        }
        ics->group_len[num_groups - 1] = (uint8_t)len;
        ics->num_windows = 8;
        ics->num_swb = t->num_swb_128[si];
        ics->tns_max_bands = t->tns_max_bands_128[si];
        src = t->swb_offset_128 + t->swb_first_128[si];
    } else {
        ics->max_sfb = (uint8_t)pc_bits(b, 6);
        ics->num_windows = 1;
        ics->num_swb = t->num_swb_1024[si];
        ics->tns_max_bands = t->tns_max_bands_1024[si];
        src = t->swb_offset_1024 + t->swb_first_1024[si];
        pred->predictor_present = (uint8_t)pc_bit1(b);
        if (pred->predictor_present) {
            if (cfg->object_type != HEAAC_AOT_AAC_MAIN) return PC_WHY_REFUSED;     /* not in AAC-LC; LTP */
            if (pc_bit1(b)) {
                const unsigned rg = pc_bits(b, 5);
                pred->predictor_reset_group = (uint8_t)rg;
                if (rg == 0 || rg > 30) return PC_WHY_REFUSED;
            }
            const int lim = ics->max_sfb < pred->pred_sfb_max ? ics->max_sfb : pred->pred_sfb_max;
            for (int sfb = 0; sfb < lim && sfb < 44; sfb++) pred->prediction_used[sfb] = (uint8_t)pc_bit1(b);
        }
    }
    ics->num_window_groups = (uint8_t)num_groups;
    const int ns = ics->num_swb < 63 ? ics->num_swb : 63;
    for (int k = 0; k <= ns; k++) ics->swb_offset[k] = src[k];
    if (ics->max_sfb > ics->num_swb) return PC_WHY_REFUSED;
    return 0;
}

/* decode_band_types: straight into the record (all bands of a section share one type, so the run ends of the host
 * parser are implied) */
PC_FN int pc_band_types(PcBits *b, HeaacToolsChannel *ch, int eight)
{
    const int nb = eight ? 3 : 5, esc = (1 << nb) - 1;
    const int max_sfb = ch->ics.max_sfb, ng = ch->ics.num_window_groups;
    int idx = 0;
    for (int g = 0; g < ng; g++) {
        int k = 0;
        while (k < max_sfb) {
            int sect_end = k, incr;
            const int bt = (int)pc_bits(b, 4);
            if (bt == 12) return PC_WHY_REFUSED;
            do {
                incr = (int)pc_bits(b, nb);
                sect_end += incr;
                /* a section that runs past max_sfb or past the unit is refused whatever follows it */
                if (b->over || sect_end > max_sfb) return PC_WHY_REFUSED;
            } while (incr == esc);
            for (; k < sect_end; k++) ch->band_type[idx++] = (uint8_t)bt;
        }
    }
    return 0;
}

/* decode_scalefactors on the C path: sf_offset = 0 (+12 for eight short) */
PC_FN int pc_scalefactors(const HeaacParseTables *t, const uint32_t *lut, PcBits *b, HeaacToolsChannel *ch, int eight,
                          int global_gain)
{
    const int sf_offset = eight ? 12 : 0;
    int off0 = global_gain, off1 = global_gain - 90, off2 = 100, noise_flag = 1;
    const int n = ch->ics.num_window_groups * ch->ics.max_sfb;
    for (int idx = 0; idx < n; idx++) {
        const int bt = ch->band_type[idx];
        if (bt == 0) continue;                        /* sf stays 0.f */
        if (bt == HEAAC_NOISE_BT && noise_flag) {
            noise_flag = 0;
            off1 += (int)pc_bits(b, 9) - 256;
            if ((unsigned)off1 > 255U) return PC_WHY_REFUSED;
            ch->sf[idx] = -t->pow2sf[off1 + sf_offset + 100];
            continue;
        }
        const int s = pc_tree(t, lut, 0, b);
        if (s < 0) return PC_WHY_REFUSED;
        if (bt == HEAAC_INTENSITY_BT || bt == HEAAC_INTENSITY_BT2) {
            off2 += s - 60;
            if ((unsigned)off2 > 255U) return PC_WHY_REFUSED;
            ch->sf[idx] = t->pow2sf[-off2 + 300];
        } else if (bt == HEAAC_NOISE_BT) {
            off1 += s - 60;
            if ((unsigned)off1 > 255U) return PC_WHY_REFUSED;
            ch->sf[idx] = -t->pow2sf[off1 + sf_offset + 100];
        } else {
            off0 += s - 60;
            if ((unsigned)off0 > 255U) return PC_WHY_REFUSED;
            ch->sf[idx] = -t->pow2sf[off0 + sf_offset];
        }
    }
    return b->over ? PC_WHY_REFUSED : 0;
}

/* decode_tns */
PC_FN int pc_tns(const HeaacAacConfig *cfg, const HeaacParseTables *t, PcBits *b, HeaacToolsChannel *ch, int eight)
{
    const int max_order = eight ? 7 : cfg->object_type == HEAAC_AOT_AAC_MAIN ? 20 : 12;
    HeaacTns *tns = &ch->tns;
    const int nw = ch->ics.num_windows;
    for (int w = 0; w < nw; w++) {
        const int n_filt = (int)pc_bits(b, 2 - eight);
        tns->n_filt[w] = (uint8_t)n_filt;
        if (!n_filt) continue;
        const int coef_res = (int)pc_bit1(b);
        for (int f = 0; f < n_filt; f++) {
            tns->length[w][f] = (uint8_t)pc_bits(b, 6 - 2 * eight);
            const int order = (int)pc_bits(b, 5 - 2 * eight);
            if (order > max_order) return PC_WHY_REFUSED;
            tns->order[w][f] = (uint8_t)order;
            if (order) {
                tns->direction[w][f] = (uint8_t)pc_bit1(b);
                const int compress = (int)pc_bit1(b);
                const int len = coef_res + 3 - compress;
                const float *map = t->tns_map[2 * compress + coef_res];
                for (int i = 0; i < order; i++) tns->coef[w][f][i] = map[pc_bits(b, len)];
            }
            if (b->over) return PC_WHY_REFUSED;
        }
    }
    return b->over ? PC_WHY_REFUSED : 0;
}

/* one quantised line of magnitude q and sign -> float: a look-up times the scalefactor */
PC_FN float pc_deq(const HeaacParseTables *t, unsigned q, int negative, float sf)
{
    const float mag = q < 16 ? t->mag[q] : t->esc[q & 8191];
    return (negative ? -mag : mag) * sf;
}

/* decode_spectrum_and_dequant without pulses; NOISE_BT bands are zeroed (the spectral tools fill them) */
PC_FN int pc_spectrum(const HeaacParseTables *t, const uint32_t *lut, PcBits *b, const HeaacToolsChannel *ch, float *coef)
{
    const HeaacToolsIcs *ics = &ch->ics;
    const int nw = ics->num_windows, max_sfb = ics->max_sfb, ng = ics->num_window_groups;
    const int c = 1024 / nw, top = ics->swb_offset[max_sfb];
    int idx = 0;
    if (top > c) return PC_WHY_REFUSED;               /* (never with the shipped band tables) */
    for (int g = 0; g < nw; g++) pc_zero(coef + g * 128 + top, c - top);
    for (int g = 0; g < ng; g++) {
        const int g_len = ics->group_len[g];
        for (int i = 0; i < max_sfb; i++, idx++) {
            const int bt = ch->band_type[idx];
            const int lo = ics->swb_offset[i], len = ics->swb_offset[i + 1] - lo;
            float *cfo = coef + lo;
            if (bt == 0 || bt >= HEAAC_NOISE_BT) {
                for (int w = 0; w < g_len; w++) pc_zero(cfo + 128 * w, len);
                continue;
            }
            const float s = ch->sf[idx];
            for (int w = 0; w < g_len; w++) {
                float *cf = cfo + 128 * w;
                if (bt <= 4) {
                    for (int k = 0; k < len; k += 4) {
                        const int code = pc_tree(t, lut, bt, b);
                        if (code < 0) return PC_WHY_REFUSED;
                        const int q0 = code / 27, q1 = code / 9 % 3, q2 = code / 3 % 3, q3 = code % 3;
                        if (bt <= 2) {
                            PC_ST4(cf + k, pc_deq(t, (unsigned)(q0 != 1), q0 < 1, s), pc_deq(t, (unsigned)(q1 != 1), q1 < 1, s),
                                   pc_deq(t, (unsigned)(q2 != 1), q2 < 1, s), pc_deq(t, (unsigned)(q3 != 1), q3 < 1, s));
                        } else {
                            /* a zero line takes the sign of the next non-zero line of its quad (none left: plus) */
                            int n0 = q0 ? (int)pc_bit1(b) : 0, n1 = q1 ? (int)pc_bit1(b) : 0;
                            int n2 = q2 ? (int)pc_bit1(b) : 0, n3 = q3 ? (int)pc_bit1(b) : 0;
                            if (!q2) n2 = n3;
                            if (!q1) n1 = n2;
                            if (!q0) n0 = n1;
                            PC_ST4(cf + k, pc_deq(t, (unsigned)q0, n0, s), pc_deq(t, (unsigned)q1, n1, s),
                                   pc_deq(t, (unsigned)q2, n2, s), pc_deq(t, (unsigned)q3, n3, s));
                        }
                    }
                } else {
                    const int mod = bt <= 6 ? 9 : bt <= 8 ? 8 : bt <= 10 ? 13 : 17;
                    for (int k = 0; k < len; k += 2) {
                        const int code = pc_tree(t, lut, bt, b);
                        if (code < 0) return PC_WHY_REFUSED;
                        const int q0 = code / mod, q1 = code % mod;
                        if (bt <= 6) {
                            const int v0 = q0 - 4, v1 = q1 - 4;
                            PC_ST2(cf + k, pc_deq(t, (unsigned)(v0 < 0 ? -v0 : v0), v0 < 0, s),
                                   pc_deq(t, (unsigned)(v1 < 0 ? -v1 : v1), v1 < 0, s));
                        } else {
                            int n0 = q0 ? (int)pc_bit1(b) : 0;
                            const int n1 = q1 ? (int)pc_bit1(b) : 0;
                            unsigned v0 = (unsigned)q0, v1 = (unsigned)q1;
                            if (bt == 11) {
                                if (!q0) n0 = n1;     /* book 11 hands the pending sign to a zero first line */
                                if (q0 == 16) {
                                    int n = 0;
                                    while (pc_bit1(b))
                                        if (++n > 8) return PC_WHY_REFUSED;
                                    v0 = (1u << (n + 4)) + pc_bits(b, n + 4);
                                }
                                if (q1 == 16) {
                                    int n = 0;
                                    while (pc_bit1(b))
                                        if (++n > 8) return PC_WHY_REFUSED;
                                    v1 = (1u << (n + 4)) + pc_bits(b, n + 4);
                                }
                            }
                            PC_ST2(cf + k, pc_deq(t, v0, n0, s), pc_deq(t, v1, n1, s));
                        }
                    }
                }
                if (b->over) return PC_WHY_REFUSED;
            }
        }
        coef += g_len << 7;
    }
    return 0;
}

/* decode_ics without pulses, gain control and apply_prediction */
PC_FN int pc_ics(const HeaacAacConfig *cfg, const HeaacParseTables *t, const uint32_t *lut, PcBits *b, int common_window,
                 HeaacToolsChannel *ch, uint32_t *win, float *coef)
{
    const int global_gain = (int)pc_bits(b, 8);
    int r;
    if (!common_window && (r = pc_ics_info(cfg, t, b, ch, win)) != 0) return r;
    const int eight = PC_WS0(*win) == 2;
    if ((r = pc_band_types(b, ch, eight)) != 0) return r;
    if ((r = pc_scalefactors(t, lut, b, ch, eight, global_gain)) != 0) return r;
    if (pc_bit1(b)) return eight ? PC_WHY_REFUSED : PC_WHY_PULSE;
    ch->tns.present = (uint8_t)pc_bit1(b);
    if (ch->tns.present && (r = pc_tns(cfg, t, b, ch, eight)) != 0) return r;
    if (pc_bit1(b)) return PC_WHY_REFUSED;            /* gain control (SSR) */
    return pc_spectrum(t, lut, b, ch, coef);
}

/* decode_dynamic_range: how many bytes of the fill element it takes */
PC_FN int pc_drc_bytes(PcBits *b)
{
    int n = 1, bands = 1;
    if (pc_bit1(b)) { pc_skip(b, 8); n++; }
    if (pc_bit1(b)) {
        int num = 0;
        do { pc_skip(b, 7); num += 7; } while (num < 64 - 7 && pc_bit1(b));
        n += num / 7;
    }
    if (pc_bit1(b)) {
        bands += (int)pc_bits(b, 4);
        pc_skip(b, 4 + 8 * bands);
        n += 1 + bands;
    }
    if (pc_bit1(b)) { pc_skip(b, 8); n++; }
    pc_skip(b, 8 * bands);
    return n + bands;
}

/* One access unit.  Returns 0 (HEAAC_PARSE_OK: *st, the records of the decoded channels, *tools and *info are what
 * heaac_aac_parse_frame_ex(cfg, st, au, size, coeff_channels, ..., NULL, info) leaves) or a PC_WHY_* reason (*st as
 * it was, the records unspecified).  *tools zeroed by the caller; coeffs 16-byte aligned. */
PC_FN int pc_walk(const HeaacAacConfig *cfg, const HeaacParseTables *t, const uint32_t *lut, HeaacAacStream *st,
                  const uint8_t *au, int size, int coeff_channels, float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                  HeaacAacFrameInfo *info)
{
    if (size <= 0) return PC_WHY_REFUSED;
    PcBits bb, *b = &bb;
    pc_init(b, au, size);
    unsigned mapped_tag = st->mapped_tag, oc = st->oc;
    if ((pc_peek32(b) >> 20) == 0xfff) {
        /* heaac_adts_parse_header and the header rules of frame_walk */
        if (size < 7) return PC_WHY_REFUSED;
        pc_skip(b, 15);                               /* sync word, id, layer */
        const int crc_abs = (int)pc_bit1(b);
        const int aot = (int)pc_bits(b, 2);
        const int sr = (int)pc_bits(b, 4);
        if (sr > 12) return PC_WHY_REFUSED;
        pc_skip(b, 1);
        const int chc = (int)pc_bits(b, 3);
        pc_skip(b, 4);
        const int flen = (int)pc_bits(b, 13);
        if (flen < 7) return PC_WHY_REFUSED;
        pc_skip(b, 11);
        const int rdb = (int)pc_bits(b, 2);
        if (!(oc & PC_OC_LOCKED)) {
            if (chc) {
                mapped_tag = 0;
                oc = (oc & PC_OC_PS) ? PC_OC_TWO : 0;
            } else {
                oc = (oc & PC_OC_TWO) | PC_OC_NONE;
            }
        }
        if (rdb != 0) return PC_WHY_REFUSED;
        if (sr != cfg->sampling_index || aot + 1 != cfg->object_type) return PC_WHY_REFUSED;
        b->pos = (crc_abs ? 7 : 9) * 8;               /* (past the end of a short unit: the next read sets `over`) */
    }
    uint32_t win0 = (uint32_t)st->window_sequence[0] | ((uint32_t)st->use_kb_window[0] << 16);
    uint32_t win1 = (uint32_t)st->window_sequence[1] | ((uint32_t)st->use_kb_window[1] << 16);
    int channels = 0, out_id = 0, sbr_bit = -1, sbr_bytes = 0, sbr_crc = 0, sbr_misplaced = 0;
    int last_che = 0, prev_type = 7;
    const int one_element = cfg->chan_config == 1 || cfg->chan_config == 2;
    int elem;
    while ((elem = (int)pc_bits(b, 3)) != 7) {
        int elem_id = (int)pc_bits(b, 4);
        if (elem == 0 || elem == 1) {                 /* SCE, CPE */
            if (channels) return PC_WHY_ELEMENT;
            if (one_element) {
                if ((elem == 1) != (cfg->chan_config == 2)) return PC_WHY_REFUSED;
                if (mapped_tag && mapped_tag != (unsigned)elem_id + 1) return PC_WHY_REFUSED;
                mapped_tag = (unsigned)elem_id + 1;
            }
            int common = 0, r;
            if (elem == 1) {
                if (coeff_channels < 2) return PC_WHY_REFUSED;
                common = (int)pc_bit1(b);
                tools->common_window = (uint8_t)common;
                if (common) {
                    if ((r = pc_ics_info(cfg, t, b, &tools->ch[0], &win0)) != 0) return r;
                    /* channel 1 takes channel 0's ics, keeping its own previous window shape */
                    win1 = (win0 & 0x00ffffffu) | (PC_KB0(win1) << 24);
                    tools->ch[1].ics = tools->ch[0].ics;
                    tools->ch[1].pred = tools->ch[0].pred;
                    const unsigned ms = pc_bits(b, 2);
                    tools->ms_present = (uint8_t)ms;
                    if (ms == 3) return PC_WHY_REFUSED;
                    const int nb = tools->ch[0].ics.num_window_groups * tools->ch[0].ics.max_sfb;
                    if (ms == 1)
                        for (int i = 0; i < nb; i++) tools->ms_mask[i] = (uint8_t)pc_bit1(b);
                    else if (ms == 2)
                        for (int i = 0; i < nb; i++) tools->ms_mask[i] = 1;
                }
            }
            if ((r = pc_ics(cfg, t, lut, b, common, &tools->ch[0], &win0, coeffs)) != 0) return r;
            if (elem == 1 && (r = pc_ics(cfg, t, lut, b, common, &tools->ch[1], &win1, coeffs + 1024)) != 0) return r;
            channels = elem + 1;
            out_id = elem_id;
        } else if (elem == 4) {                       /* DSE */
            const int align = (int)pc_bit1(b);
            int count = (int)pc_bits(b, 8);
            if (count == 255) count += (int)pc_bits(b, 8);
            if (b->over) return PC_WHY_REFUSED;
            if (align) b->pos = (b->pos + 7) & ~7;
            if (pc_left(b) < 8 * count) return PC_WHY_REFUSED;
            b->pos += 8 * count;
        } else if (elem == 6) {                       /* FIL */
            if (elem_id == 15) elem_id += (int)pc_bits(b, 8) - 1;
            if (b->over || pc_left(b) < 8 * elem_id) return PC_WHY_REFUSED;
            int cnt = elem_id, at = -1, bytes = 0, crc = 0;
            while (cnt > 0) {
                const int type = (int)pc_bits(b, 4);
                if (type == 0xb) {                    /* EXT_DYNAMIC_RANGE */
                    cnt -= pc_drc_bytes(b);
                    if (b->over) return PC_WHY_REFUSED;
                    continue;
                }
                if (type == 0xd || type == 0xe) {     /* EXT_SBR_DATA, EXT_SBR_DATA_CRC */
                    at = b->pos;
                    bytes = cnt;
                    crc = type == 0xe;
                }
                pc_skip(b, 8 * cnt - 4);
                cnt = 0;
            }
            if (at >= 0) {
                if (!last_che) return PC_WHY_REFUSED;
                if (sbr_bit >= 0) return PC_WHY_REFUSED;
                sbr_bit = at;
                sbr_bytes = bytes;
                sbr_crc = crc;
                sbr_misplaced = prev_type != 0 && prev_type != 1;
                if (cfg->sbr != 0 && cfg->ps == -1 && cfg->chan_config == 1 && !(oc & (PC_OC_LOCKED | PC_OC_PS | PC_OC_TWO))) {
                    oc |= PC_OC_PS | PC_OC_TWO;
                    mapped_tag = 0;
                }
            }
        } else {
            return PC_WHY_ELEMENT;                    /* CCE, LFE, PCE */
        }
        if (elem < 4) last_che = elem + 1;
        prev_type = elem;
        if (b->over) return PC_WHY_REFUSED;
        if (pc_left(b) < 3) return PC_WHY_REFUSED;
    }
    if (!channels || b->over) return PC_WHY_REFUSED;
    /* the unit parses: commit */
    ics[0].window_sequence[0] = (uint8_t)win0;         ics[0].window_sequence[1] = (uint8_t)(win0 >> 8);
    ics[0].use_kb_window[0] = (uint8_t)(win0 >> 16);   ics[0].use_kb_window[1] = (uint8_t)(win0 >> 24);
    st->window_sequence[0] = (uint8_t)win0;
    st->use_kb_window[0] = (uint8_t)(win0 >> 16);
    if (channels == 2) {
        ics[1].window_sequence[0] = (uint8_t)win1;         ics[1].window_sequence[1] = (uint8_t)(win1 >> 8);
        ics[1].use_kb_window[0] = (uint8_t)(win1 >> 16);   ics[1].use_kb_window[1] = (uint8_t)(win1 >> 24);
        st->window_sequence[1] = (uint8_t)win1;
        st->use_kb_window[1] = (uint8_t)(win1 >> 16);
    }
    if (!(oc & PC_OC_NONE)) oc |= PC_OC_LOCKED;
    st->mapped_tag = (uint8_t)mapped_tag;
    st->oc = (uint8_t)oc;
    info->channels = channels;
    info->bits_consumed = b->pos;
    info->sbr_payload_bit = sbr_bit;
    info->sbr_payload_bytes = sbr_bytes;
    info->sbr_crc = sbr_crc;
    info->elem_id = out_id;
    info->n_cce = 0;
    info->sbr_misplaced = sbr_misplaced;
    info->refused = 0;
    return 0;
}

#endif /* HEAAC_PARSE_CORE_H */
