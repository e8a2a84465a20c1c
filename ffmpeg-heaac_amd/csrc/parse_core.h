/* parse_core.h -- the element syntax of an AAC access unit (include/heaac_parse.h; ISO/IEC 14496-3 tables 4.4 - 4.54
 * as the reference's aacdec.c reads them), written once for the host and the device.
 *
 * The pc_* readers are the one writing of the individual channel stream, the channel pair's head, the data stream and
 * fill elements and the ADTS header rules: which bits are read in which order, every check, and how a quantised line
 * becomes a float.  They take their tables, the unit and the window history by pointer and perform no I/O.  The host
 * parser (aac_parse.c: frame_walk, layout_walk, read_cce) calls them with a PcHost record, through which they report the
 * exact HEAAC_PARSE_ERR_* status and how far the reference's decoders had got, and read pulse data; what only the host
 * does -- the HEAAC_REFUSED_* rules, pulse_add through libm, coupling, program config and LFE elements, layouts --
 * stays there.
 *
 * pc_walk is the element loop of heaac_aac_parse_device: one SCE or one CPE per unit, AAC-LC / AAC-Main, data stream
 * and fill elements skipped, an ADTS header in front.  k_parse_streams.hip instantiates it one lane per unit, and for the host
 * as heaac_debug_aac_parse_core (include/heaac_debug.h), where it is tested, fuzzed and debugged.  It passes NULL for
 * the PcHost record and never decides a refusal: wherever the host parser would return anything but HEAAC_PARSE_OK it
 * gives the unit up (a PC_WHY_* reason, status HEAAC_PARSE_DEFERRED) and the caller hands it to the host parser; so
 * does a unit with pulse data (pulse_add goes through libm's cbrtf on an arbitrary float) and one with a CCE, PCE, LFE
 * or a second SCE / CPE.
 *
 * A channel's window history is one uint32_t laid out as HeaacIcs: every loop loads it from the stream row, the
 * readers move it on, and the loop stores it back where its own policy commits (pc_walk: on OK only; the records of a
 * unit that is given up are unspecified).
 *
 * The caller zeroes the unit's HeaacToolsFrame ahead of the readers.
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

/* HeaacAacStream.oc (see pc_adts); the raw / AudioSpecificConfig path configures once, at init (:430), and never again */
#define PC_OC_LOCKED 1u               /* output_configured == OC_LOCKED */
#define PC_OC_NONE   2u               /* an ADTS header without a channel configuration left OC_NONE: the unit does not lock */
#define PC_OC_PS     4u               /* m4ac.ps is 1: the implicit-PS re-configure has run (an ADTS header sets it back to -1) */
#define PC_OC_TWO    8u               /* the last output_configure counted two channels for the SCE (it ran with ps == 1) */

/* ---- bit reader: MSB first; reading past the end yields zeros and sets `over`; the unit is read eight bytes at a
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
PC_FN unsigned pc_peek(PcBits *b, int n) { return n > 0 ? pc_peek32(b) >> (32 - n) : 0; }
PC_FN int pc_left(const PcBits *b) { return b->size_bits - b->pos; }

/* one code of a book of parse_bits.h's tree_build: -1 for a prefix that is no code of the book.  `lut` = the twelve prefix tables
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

/* What the host parser keeps on top of the syntax: the exact status of a refusal, how far the reference's element
 * decoders had got by then (decoder state they have moved stays moved: the window history of decode_ics_info, the noise
 * generator of decode_spectrum_and_dequant, the predictors of apply_prediction), and the pulse data of the channel in
 * work, which the host applies through libm.  `as_reference` is set where the refusal is one the reference makes at the
 * same bit of the unit; the checks of this parser alone (a read past the end that the reference's unchecked reader would
 * run through, the layouts it does not take) leave it clear.  The device and heaac_debug_aac_parse_core pass a constant
 * NULL for it: nothing of it is left in their code, and a unit with pulse data is given up. */
typedef struct PcHost {
    int status;             /* the HEAAC_PARSE_ERR_* of the refusal */
    uint8_t ics[2];         /* per channel: 0 window history untouched, 1 moved on to this unit's, 2 cleared */
    uint8_t decoded[2];     /* decode_ics has returned 0 for the channel */
    uint8_t predicted[2];   /* apply_prediction has run on it */
    uint8_t as_reference;
    uint8_t ref_overread;   /* ... and it is one of the reference's own end-of-unit checks */
    int noise_stop[2];      /* channel not decoded: bands [0, noise_stop) have been through the spectrum loop */
    int num_pulse[2], pulse_pos[2][4], pulse_amp[2][4];   /* per channel: pulse data read, for the host to add */
} PcHost;

/* every refusal leaves through here; ref: 0 this parser's own check, 1 the reference's, 2 its end-of-unit check */
PC_FN int pc_refuse(PcHost *pg, int status, int ref)
{
    if (pg) {
        pg->status = status;
        if (ref) pg->as_reference = 1;
        if (ref == 2) pg->ref_overread = 1;
    }
    return PC_WHY_REFUSED;
}
#define PC_REF_OVERREAD(pg) pc_refuse(pg, HEAAC_PARSE_ERR_OVERREAD, 2)

/* decode_ics_info + decode_prediction (aacdec.c:622-742) of channel c; *win: the channel's history moves on to this
 * unit's.  Every refusal in here is the reference's, and each of them clears the whole IndividualChannelStream (memset,
 * aacdec.c:650, 687, 692, 696, 705): the window history with it.  *ch zeroed by the caller. */
PC_FN int pc_ics_info(const HeaacAacConfig *cfg, const HeaacParseTables *t, PcBits *b, HeaacToolsChannel *ch, uint32_t *win,
                      PcHost *pg, int c)
{
    const int si = cfg->sampling_index;
    HeaacToolsIcs *ics = &ch->ics;
    HeaacPrediction *pred = &ch->pred;
    if (pg) pg->ics[c] = 2;
    if (pc_bit1(b)) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);            /* reserved bit */
    const unsigned ws = pc_bits(b, 2), kb = pc_bit1(b);
    *win = ws | (PC_WS0(*win) << 8) | (kb << 16) | (PC_KB0(*win) << 24);
    int num_groups = 1;
    ics->num_window_groups = 1;
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
        ics->num_window_groups = (uint8_t)num_groups;
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
    }
    const int ns = ics->num_swb < 63 ? ics->num_swb : 63;
    for (int k = 0; k <= ns; k++) ics->swb_offset[k] = src[k];
    if (ws != 2) {
        pred->predictor_present = (uint8_t)pc_bit1(b);
        if (pred->predictor_present) {
            if (cfg->object_type != HEAAC_AOT_AAC_MAIN)  /* prediction is not allowed in AAC-LC; elsewhere it is LTP */
                return pc_refuse(pg, cfg->object_type == HEAAC_AOT_AAC_LC ? HEAAC_PARSE_ERR_DATA : HEAAC_PARSE_ERR_UNSUPPORTED, 1);
            if (pc_bit1(b)) {
                const unsigned rg = pc_bits(b, 5);
                pred->predictor_reset_group = (uint8_t)rg;
                if (rg == 0 || rg > 30) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
            }
            const int lim = ics->max_sfb < pred->pred_sfb_max ? ics->max_sfb : pred->pred_sfb_max;
            for (int sfb = 0; sfb < lim && sfb < 44; sfb++) pred->prediction_used[sfb] = (uint8_t)pc_bit1(b);
        }
    }
    if (ics->max_sfb > ics->num_swb) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
    if (pg) pg->ics[c] = 1;
    return 0;
}

/* decode_band_types (:755-801): straight into the record (all bands of a section share one type).  Past the end the
 * reference reads the zeros of its input padding, leaves the escape run and fails its get_bits_left() < 0 check
 * (:778-781): the same refusal, taken here without the walk, so the run is bounded by the unit's bits. */
PC_FN int pc_band_types(PcBits *b, HeaacToolsChannel *ch, int eight, PcHost *pg)
{
    const int nb = eight ? 3 : 5, esc = (1 << nb) - 1;
    const int max_sfb = ch->ics.max_sfb, ng = ch->ics.num_window_groups;
    int idx = 0;
    for (int g = 0; g < ng; g++) {
        int k = 0;
        while (k < max_sfb) {
            int sect_end = k, incr;
            const int bt = (int)pc_bits(b, 4);
            if (bt == 12) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
            do {
                incr = (int)pc_bits(b, nb);
                sect_end += incr;
                if (b->over) return PC_REF_OVERREAD(pg);
            } while (incr == esc);
            if (sect_end > max_sfb) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
            for (; k < sect_end; k++) ch->band_type[idx++] = (uint8_t)bt;
        }
    }
    return 0;
}

/* decode_scalefactors (:815-873) on the C path: sf_offset = 0 (+12 for eight short) */
PC_FN int pc_scalefactors(const HeaacParseTables *t, const uint32_t *lut, PcBits *b, HeaacToolsChannel *ch, int eight,
                          int global_gain, PcHost *pg)
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
            if ((unsigned)off1 > 255U) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
            ch->sf[idx] = -t->pow2sf[off1 + sf_offset + 100];
            continue;
        }
        const int s = pc_tree(t, lut, 0, b);
        if (s < 0) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 0);
        if (bt == HEAAC_INTENSITY_BT || bt == HEAAC_INTENSITY_BT2) {
            off2 += s - 60;
            if ((unsigned)off2 > 255U) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
            ch->sf[idx] = t->pow2sf[-off2 + 300];
        } else if (bt == HEAAC_NOISE_BT) {
            off1 += s - 60;
            if ((unsigned)off1 > 255U) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
            ch->sf[idx] = -t->pow2sf[off1 + sf_offset + 100];
        } else {
            off0 += s - 60;
            if ((unsigned)off0 > 255U) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
            ch->sf[idx] = -t->pow2sf[off0 + sf_offset];
        }
    }
    return b->over ? pc_refuse(pg, HEAAC_PARSE_ERR_OVERREAD, 0) : 0;
}

/* decode_pulses (:878-900), host only: into pg, for the caller to apply */
PC_FN int pc_pulses(PcBits *b, const HeaacToolsIcs *ics, PcHost *pg, int c)
{
    const int num_pulse = (int)pc_bits(b, 2) + 1;
    const int swb = (int)pc_bits(b, 6);
    if (swb >= ics->num_swb) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
    int pos = ics->swb_offset[swb];
    for (int i = 0; i < num_pulse; i++) {
        pos += (int)pc_bits(b, 5);
        if (pos > 1023) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
        pg->pulse_pos[c][i] = pos;
        pg->pulse_amp[c][i] = (int)pc_bits(b, 4);
    }
    pg->num_pulse[c] = num_pulse;
    return 0;
}

/* decode_tns (:907-945) */
PC_FN int pc_tns(const HeaacAacConfig *cfg, const HeaacParseTables *t, PcBits *b, HeaacToolsChannel *ch, int eight, PcHost *pg)
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
            if (order > max_order) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);      /* order[w][f] stays 0 */
            tns->order[w][f] = (uint8_t)order;
            if (order) {
                tns->direction[w][f] = (uint8_t)pc_bit1(b);
                const int compress = (int)pc_bit1(b);
                const int len = coef_res + 3 - compress;
                const float *map = t->tns_map[2 * compress + coef_res];
                for (int i = 0; i < order; i++) tns->coef[w][f][i] = map[pc_bits(b, len)];
            }
        }
    }
    return b->over ? pc_refuse(pg, HEAAC_PARSE_ERR_OVERREAD, 0) : 0;
}

/* one quantised line of magnitude q (< 16 from the books, up to 8191 from an escape) and sign -> float: a look-up
 * (mag(q) = q^(4/3) as a float, cbrtf(q) * q for an escape value) times the scalefactor */
PC_FN float pc_deq(const HeaacParseTables *t, unsigned q, int negative, float sf)
{
    const float mag = q < 16 ? t->mag[q] : t->esc[q & 8191];
    return (negative ? -mag : mag) * sf;
}

/* decode_spectrum_and_dequant (:988-1245) of channel c without the pulses; NOISE_BT bands are zeroed (the spectral
 * tools fill them) */
PC_FN int pc_spectrum(const HeaacParseTables *t, const uint32_t *lut, PcBits *b, const HeaacToolsChannel *ch, float *coef,
                      PcHost *pg, int c)
{
    const HeaacToolsIcs *ics = &ch->ics;
    const int nw = ics->num_windows, max_sfb = ics->max_sfb, ng = ics->num_window_groups;
    const int cn = 1024 / nw, top = ics->swb_offset[max_sfb];
    int idx = 0;
    if (top > cn) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 0);      /* (never with the shipped band tables) */
    for (int g = 0; g < nw; g++) pc_zero(coef + g * 128 + top, cn - top);
    for (int g = 0; g < ng; g++) {
        const int g_len = ics->group_len[g];
        for (int i = 0; i < max_sfb; i++, idx++) {
            const int bt = ch->band_type[idx];
            const int lo = ics->swb_offset[i], len = ics->swb_offset[i + 1] - lo;
            float *cfo = coef + lo;
            if (pg) pg->noise_stop[c] = idx;          /* the noise bands in front of this one have drawn their numbers */
            if (bt == 0 || bt >= HEAAC_NOISE_BT) {
                for (int w = 0; w < g_len; w++) pc_zero(cfo + 128 * w, len);
                continue;
            }
            const float s = ch->sf[idx];
            for (int w = 0; w < g_len; w++) {
                float *cf = cfo + 128 * w;
                if (bt <= 4) {
                    /* quads: books 1, 2 signed (-1..1), books 3, 4 unsigned (0..2) + sign bits */
                    for (int k = 0; k < len; k += 4) {
                        const int code = pc_tree(t, lut, bt, b);
                        if (code < 0) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 0);
                        const int q0 = code / 27, q1 = code / 9 % 3, q2 = code / 3 % 3, q3 = code % 3;
                        if (bt <= 2) {
                            PC_ST4(cf + k, pc_deq(t, (unsigned)(q0 != 1), q0 < 1, s), pc_deq(t, (unsigned)(q1 != 1), q1 < 1, s),
                                   pc_deq(t, (unsigned)(q2 != 1), q2 < 1, s), pc_deq(t, (unsigned)(q3 != 1), q3 < 1, s));
                        } else {
                            /* VMUL4S (:949-972) flips the scalefactor's sign by the sign bit at the head of the pending
                             * ones and moves on only behind a non-zero line: a zero line takes the sign of the NEXT
                             * non-zero line of its quad (none left: plus) -- the sign of a zero, which no value
                             * downstream depends on, kept for the coefficients' bit pattern */
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
                    /* pairs: books 5, 6 signed (-4..4); 7, 8 (0..7), 9, 10 (0..12), 11 (0..16, 16 = escape) unsigned */
                    const int mod = bt <= 6 ? 9 : bt <= 8 ? 8 : bt <= 10 ? 13 : 17;
                    for (int k = 0; k < len; k += 2) {
                        const int code = pc_tree(t, lut, bt, b);
                        if (code < 0) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 0);
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
                                /* book 11 ORs the pending sign bit into a zero first line as well (:1199-1201); books
                                 * 7 ... 10 (VMUL2S :935-947) do not.  escape_sequence: N ones, a zero, then N + 4 bits
                                 * (:1174-1197); more than 8 ones is the reference's "ESC overflow" (:1187-1190) */
                                if (!q0) n0 = n1;
                                if (q0 == 16) {
                                    int n = 0;
                                    while (pc_bit1(b))
                                        if (++n > 8) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
                                    v0 = (1u << (n + 4)) + pc_bits(b, n + 4);
                                }
                                if (q1 == 16) {
                                    int n = 0;
                                    while (pc_bit1(b))
                                        if (++n > 8) {
                                            cf[k] = pc_deq(t, v0, n0, s);              /* (the reference has stored the first line) */
                                            return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
                                        }
                                    v1 = (1u << (n + 4)) + pc_bits(b, n + 4);
                                }
                            }
                            PC_ST2(cf + k, pc_deq(t, v0, n0, s), pc_deq(t, v1, n1, s));
                        }
                    }
                }
                if (b->over) return pc_refuse(pg, HEAAC_PARSE_ERR_OVERREAD, 0);
            }
        }
        coef += g_len << 7;
    }
    return 0;
}

/* decode_ics (:1334-1388) of channel c without gain control, apply_prediction (a GPU stage) and the pulses' effect:
 * with pg (zeroed by the caller ahead of the element) they are read into it for the caller to add once the channel
 * is decoded, without it the unit is given up */
PC_FN int pc_ics(const HeaacAacConfig *cfg, const HeaacParseTables *t, const uint32_t *lut, PcBits *b, int common_window,
                 HeaacToolsChannel *ch, uint32_t *win, float *coef, PcHost *pg, int c)
{
    const int global_gain = (int)pc_bits(b, 8);
    int r;
    if (!common_window && (r = pc_ics_info(cfg, t, b, ch, win, pg, c)) != 0) return r;
    const int eight = PC_WS0(*win) == 2;
    if ((r = pc_band_types(b, ch, eight, pg)) != 0) return r;
    if ((r = pc_scalefactors(t, lut, b, ch, eight, global_gain, pg)) != 0) return r;
    if (pc_bit1(b)) {
        if (eight) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);      /* pulse tool not allowed in eight short sequence */
        if (!pg) return PC_WHY_PULSE;
        if ((r = pc_pulses(b, &ch->ics, pg, c)) != 0) return r;
    }
    ch->tns.present = (uint8_t)pc_bit1(b);
    if (ch->tns.present && (r = pc_tns(cfg, t, b, ch, eight, pg)) != 0) return r;
    if (pc_bit1(b)) return pc_refuse(pg, HEAAC_PARSE_ERR_UNSUPPORTED, 1);      /* gain control (SSR) */
    if (pg) pg->noise_stop[c] = 0;
    if ((r = pc_spectrum(t, lut, b, ch, coef, pg, c)) != 0) return r;
    if (pg) {
        pg->decoded[c] = 1;
        /* apply_prediction inside decode_ics (:1381-1382) */
        if (cfg->object_type == HEAAC_AOT_AAC_MAIN && !common_window) pg->predicted[c] = 1;
    }
    return 0;
}

/* single_channel_element (pair 0; so is an LFE, and the channel of a coupling element) or channel_pair_element
 * (decode_cpe, :1453-1492) behind its instance tag, without the spectral tools (GPU stages); win[2] = the channels'
 * window history, coeffs [2][1024]; channel 1 of either is untouched for a single channel */
PC_FN int pc_che(const HeaacAacConfig *cfg, const HeaacParseTables *t, const uint32_t *lut, PcBits *b, int pair,
                 HeaacToolsFrame *tools, uint32_t *win, float *coeffs, PcHost *pg)
{
    int r, common = 0;
    if (pair) {
        common = (int)pc_bit1(b);
        tools->common_window = (uint8_t)common;
    }
    if (common) {
        if ((r = pc_ics_info(cfg, t, b, &tools->ch[0], &win[0], pg, 0)) != 0) return r;
        /* channel 1 takes channel 0's ics, keeping its own previous window shape (:1462-1464) */
        win[1] = (win[0] & 0x00ffffffu) | (PC_KB0(win[1]) << 24);
        if (pg) pg->ics[1] = 1;
        tools->ch[1].ics = tools->ch[0].ics;
        tools->ch[1].pred = tools->ch[0].pred;
        const unsigned ms = pc_bits(b, 2);
        tools->ms_present = (uint8_t)ms;
        if (ms == 3) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
        const int nb = tools->ch[0].ics.num_window_groups * tools->ch[0].ics.max_sfb;
        if (ms == 1)
            for (int i = 0; i < nb; i++) tools->ms_mask[i] = (uint8_t)pc_bit1(b);
        else if (ms == 2)
            for (int i = 0; i < nb; i++) tools->ms_mask[i] = 1;
    }
    if ((r = pc_ics(cfg, t, lut, b, common, &tools->ch[0], &win[0], coeffs, pg, 0)) != 0) return r;
    if (pair && (r = pc_ics(cfg, t, lut, b, common, &tools->ch[1], &win[1], coeffs + 1024, pg, 1)) != 0) return r;
    /* apply_prediction at the end of decode_cpe (:1486-1489) */
    if (pg && common && cfg->object_type == HEAAC_AOT_AAC_MAIN) pg->predicted[0] = pg->predicted[1] = 1;
    return 0;
}

/* a channel's window history: out of the stream row, and into the unit's record and back where the caller commits */
PC_FN uint32_t pc_win_load(unsigned window_sequence, unsigned use_kb_window)
{
    return window_sequence | (use_kb_window << 16);
}
PC_FN void pc_win_store(uint32_t win, HeaacIcs *ics, uint8_t *window_sequence, uint8_t *use_kb_window)
{
    ics->window_sequence[0] = (uint8_t)win;        ics->window_sequence[1] = (uint8_t)(win >> 8);
    ics->use_kb_window[0] = (uint8_t)(win >> 16);  ics->use_kb_window[1] = (uint8_t)(win >> 24);
    *window_sequence = (uint8_t)win;
    *use_kb_window = (uint8_t)(win >> 16);
}

/* data_stream_element behind its tag: skipped (skip_data_stream_element, :602-620) */
PC_FN int pc_dse(PcBits *b, PcHost *pg)
{
    const int align = (int)pc_bit1(b);
    int count = (int)pc_bits(b, 8);
    if (count == 255) count += (int)pc_bits(b, 8);
    if (align) b->pos = (b->pos + 7) & ~7;
    if (pc_left(b) < 8 * count) return pc_refuse(pg, HEAAC_PARSE_ERR_OVERREAD, 0);
    b->pos += 8 * count;
    return 0;
}

/* decode_dynamic_range (:1596-1641) behind the payload's type nibble: nothing of it is used on this path, but it says
 * how many bytes of the fill element it takes -- the one extension payload that does not take all that is left */
PC_FN int pc_drc_bytes(PcBits *b)
{
    int n = 1, bands = 1;
    if (pc_bit1(b)) { pc_skip(b, 8); n++; }           /* pce_instance_tag, reserved */
    if (pc_bit1(b)) {                                 /* excluded channels (decode_drc_channel_exclusions :1575-1587) */
        int num = 0;
        do { pc_skip(b, 7); num += 7; } while (num < 64 - 7 && pc_bit1(b));
        n += num / 7;
    }
    if (pc_bit1(b)) {                                 /* band_incr, interpolation_scheme, band_top[] */
        bands += (int)pc_bits(b, 4);
        pc_skip(b, 4 + 8 * bands);
        n += 1 + bands;
    }
    if (pc_bit1(b)) { pc_skip(b, 8); n++; }           /* prog_ref_level */
    pc_skip(b, 8 * bands);                            /* dyn_rng_sgn, dyn_rng_ctl */
    return n + bands;
}

/* fill_element behind its count nibble `cnt`: the escape count, the reference's check that the unit holds that many
 * bytes (:2053-2056), then extension payloads until they are used up (decode_extension_payload :1650-1690).  *sbr_bit =
 * where an SBR payload starts (behind its type nibble; it takes all that is left, :1044-1050), -1 for none. */
PC_FN int pc_fil(PcBits *b, int cnt, int *sbr_bit, int *sbr_bytes, int *sbr_crc, PcHost *pg)
{
    if (cnt == 15) cnt += (int)pc_bits(b, 8) - 1;
    if (pc_left(b) < 8 * cnt) return PC_REF_OVERREAD(pg);
    *sbr_bit = -1;
    while (cnt > 0) {
        const int type = (int)pc_bits(b, 4);
        if (type == 0xb) {                            /* EXT_DYNAMIC_RANGE */
            cnt -= pc_drc_bytes(b);
            continue;
        }
        if (type == 0xd || type == 0xe) {             /* EXT_SBR_DATA, EXT_SBR_DATA_CRC */
            *sbr_bit = b->pos;
            *sbr_bytes = cnt;
            *sbr_crc = type == 0xe;
        }
        pc_skip(b, 8 * cnt - 4);
        cnt = 0;
    }
    return 0;
}

/* adts_fixed_header + adts_variable_header at the cursor: the fields as sent, written on success only.  Returns the
 * header's bytes (7, or 9 with a CRC) or -1 no sync word, -2 reserved rate, -3 a frame shorter than its header.
 * sample_rate, samples and bit_rate are heaac_adts_parse_header's. */
PC_FN int pc_adts_header(PcBits *b, HeaacAdtsHeader *h)
{
    if (pc_bits(b, 12) != 0xfff) return -1;
    pc_skip(b, 3);                                    /* id, layer */
    const int crc_abs = (int)pc_bit1(b);
    const int aot = (int)pc_bits(b, 2);
    const int sr = (int)pc_bits(b, 4);
    if (sr > 12) return -2;
    pc_skip(b, 1);                                    /* private_bit */
    const int ch = (int)pc_bits(b, 3);
    pc_skip(b, 4);                                    /* original/copy, home, copyright id bit + start */
    const int flen = (int)pc_bits(b, 13);
    if (flen < 7) return -3;
    pc_skip(b, 11);                                   /* adts_buffer_fullness */
    const int rdb = (int)pc_bits(b, 2);
    h->object_type = aot + 1;
    h->chan_config = ch;
    h->crc_absent = crc_abs;
    h->num_aac_frames = rdb + 1;
    h->sampling_index = sr;
    h->frame_length = flen;
    return crc_abs ? 7 : 9;
}

/* An ADTS header in front of the raw data block (aacdec.c:1988-1997), the cursor at its sync word.  *oc (NULL: a
 * layout's stream, which has no such rules) is HeaacAacStream.oc, what the reference's output configuration has done
 * to a one-element stream: until a unit has decoded (PC_OC_LOCKED, aac_decode_frame :2100-2101) every header runs
 * output_configure again (:1942-1955) -- with the channel configuration (the tag map cleared; the SCE counted twice
 * where ps is 1 just now) or leaving OC_NONE without one; then ps = -1.  parse_adts_frame_header (:1935-1971) takes
 * rate and object type from every header and refuses more than one raw data block per frame; `cfg` is the caller's
 * (read-only, shared by a batch): a header that contradicts it would be dequantised against the wrong band tables, so
 * it is refused instead. */
PC_FN int pc_adts(const HeaacAacConfig *cfg, PcBits *b, uint8_t *mapped_tag, uint8_t *oc, PcHost *pg)
{
    HeaacAdtsHeader h;
    if (b->size_bytes < 7 || pc_adts_header(b, &h) < 0) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 0);
    if (oc && !(*oc & PC_OC_LOCKED)) {
        if (h.chan_config) {
            *mapped_tag = 0;
            *oc = (*oc & PC_OC_PS) ? PC_OC_TWO : 0;
        } else {
            *oc = (uint8_t)((*oc & PC_OC_TWO) | PC_OC_NONE);
        }
    }
    if (h.num_aac_frames != 1) return pc_refuse(pg, HEAAC_PARSE_ERR_UNSUPPORTED, 0);
    if (h.sampling_index != cfg->sampling_index || h.object_type != cfg->object_type) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 0);
    b->pos = (h.crc_absent ? 7 : 9) * 8;              /* (past the end of a short unit: the next read sets `over`) */
    return 0;
}

/* decode_extension_payload (:1666-1673) at an SBR payload: implicit PS in a one-channel stream before the lock sets
 * ps = 1 and runs output_configure again -- the tag the SCE was just mapped to is forgotten */
PC_FN void pc_implicit_ps(const HeaacAacConfig *cfg, uint8_t *mapped_tag, uint8_t *oc)
{
    if (cfg->sbr != 0 && cfg->ps == -1 && cfg->chan_config == 1 && !(*oc & (PC_OC_LOCKED | PC_OC_PS | PC_OC_TWO))) {
        *oc |= PC_OC_PS | PC_OC_TWO;
        *mapped_tag = 0;
    }
}

/* get_che (aacdec.c:113-177) for a stream of channel configuration 1 or 2: the configuration's one element -- an SCE
 * for 1, a CPE for 2 -- is mapped to the instance tag it is first met with; anything else, a second element of the
 * unit (its tag counts as seen, the next one is not mapped) and the same element under another tag in a later unit
 * find no element allocated and fail the unit there (:2011-2015), with nothing of their own read. */
PC_FN int pc_output_element(const HeaacAacConfig *cfg, uint8_t *mapped_tag, int type, int tag, int have_one, PcHost *pg)
{
    const int one_element = cfg->chan_config == 1 || cfg->chan_config == 2;
    if (have_one) return pc_refuse(pg, HEAAC_PARSE_ERR_UNSUPPORTED, one_element);
    if (one_element) {
        if ((type == 1) != (cfg->chan_config == 2)) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
        if (*mapped_tag && *mapped_tag != tag + 1) return pc_refuse(pg, HEAAC_PARSE_ERR_DATA, 1);
        *mapped_tag = (uint8_t)(tag + 1);             /* (only an output_configure clears it: pc_adts, pc_implicit_ps) */
    }
    return 0;
}

/* One access unit on the device's terms: one SCE or one CPE, data stream and fill elements, an ADTS header in front.
 * Returns 0 (HEAAC_PARSE_OK: *st, the records of the decoded channels, *tools and *info are what
 * heaac_aac_parse_frame_ex(cfg, st, au, size, coeff_channels, ..., NULL, info) leaves) or a PC_WHY_* reason (*st as
 * it was, the records unspecified).  *tools zeroed by the caller; coeffs 16-byte aligned. */
PC_FN int pc_walk(const HeaacAacConfig *cfg, const HeaacParseTables *t, const uint32_t *lut, HeaacAacStream *st,
                  const uint8_t *au, int size, int coeff_channels, float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                  HeaacAacFrameInfo *info)
{
    if (size <= 0) return PC_WHY_REFUSED;
    PcBits bb, *b = &bb;
    pc_init(b, au, size);
    uint8_t mapped_tag = st->mapped_tag, oc = st->oc;
    int r;
    if ((pc_peek32(b) >> 20) == 0xfff && (r = pc_adts(cfg, b, &mapped_tag, &oc, NULL)) != 0) return r;
    uint32_t win[2] = { pc_win_load(st->window_sequence[0], st->use_kb_window[0]),
                        pc_win_load(st->window_sequence[1], st->use_kb_window[1]) };
    int channels = 0, out_id = 0, sbr_bit = -1, sbr_bytes = 0, sbr_crc = 0, sbr_misplaced = 0;
    int last_che = 0, prev_type = 7;
    int elem;
    while ((elem = (int)pc_bits(b, 3)) != 7) {
        const int elem_id = (int)pc_bits(b, 4);
        if (elem == 0 || elem == 1) {                 /* SCE, CPE */
            if (channels) return PC_WHY_ELEMENT;
            if ((r = pc_output_element(cfg, &mapped_tag, elem, elem_id, 0, NULL)) != 0) return r;
            if (elem == 1 && coeff_channels < 2) return PC_WHY_REFUSED;
            if ((r = pc_che(cfg, t, lut, b, elem, tools, win, coeffs, NULL)) != 0) return r;
            channels = elem + 1;
            out_id = elem_id;
        } else if (elem == 4) {                       /* DSE */
            if ((r = pc_dse(b, NULL)) != 0) return r;
        } else if (elem == 6) {                       /* FIL */
            int at, bytes = 0, crc = 0;
            if ((r = pc_fil(b, elem_id, &at, &bytes, &crc, NULL)) != 0) return r;
            if (at >= 0) {
                if (!last_che) return PC_WHY_REFUSED;
                if (sbr_bit >= 0) return PC_WHY_REFUSED;
                sbr_bit = at;
                sbr_bytes = bytes;
                sbr_crc = crc;
                sbr_misplaced = prev_type != 0 && prev_type != 1;
                pc_implicit_ps(cfg, &mapped_tag, &oc);
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
    for (int c = 0; c < channels; c++) pc_win_store(win[c], &ics[c], &st->window_sequence[c], &st->use_kb_window[c]);
    if (!(oc & PC_OC_NONE)) oc |= PC_OC_LOCKED;
    st->mapped_tag = mapped_tag;
    st->oc = oc;
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
