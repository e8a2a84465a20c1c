/* aac_parse.c -- host-side AAC access-unit parser (include/heaac_parse.h).
 *
 * The element syntax -- which bits are read in which order (ISO/IEC 14496-3 tables 4.4 - 4.54 as aacdec.c reads them),
 * every check, and how a quantised line becomes a float -- is written once, in parse_core.h, for this parser and for
 * the device's; the tables are parse_tables.c's.  Here is what only the host does: AudioSpecificConfig and program
 * config elements, the element loops of a one-element stream (frame_walk) and of a layout (layout_walk) with coupling
 * and LFE elements, the pulses (pulse_add re-quantises a line as aacdec.c:1222-1236 does, through libm), what a refused
 * unit leaves behind (HEAAC_REFUSED_*), the batch over threads.  One pass per element writes straight into the records
 * of the batched GPU entry points.
 */
#include <math.h>
#include <pthread.h>
#include <string.h>
#include <unistd.h>
#include "heaac_parse.h"
#include "parse_core.h"

/* ------------------------------------------------------------------------------------------ */
/* AudioSpecificConfig, ADTS                                                                     */
/* ------------------------------------------------------------------------------------------ */
static const int k_rates[16] = { 96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000,
                                 11025, 8000, 7350, 0, 0, 0 };

static int get_object_type(PcBits *b)
{
    int t = (int)pc_bits(b, 5);
    if (t == 31) t = 32 + (int)pc_bits(b, 6);
    return t;
}
static int get_sample_rate(PcBits *b, int *index)
{
    *index = (int)pc_bits(b, 4);
    return *index == 0x0f ? (int)pc_bits(b, 24) : k_rates[*index];
}

int heaac_asc_parse(HeaacAacConfig *c, const uint8_t *buf, int size)
{
    if (!c || !buf || size <= 0) return HEAAC_PARSE_ERR_ARG;
    PcBits b;
    pc_init(&b, buf, size);
    memset(c, 0, sizeof(*c));
    c->object_type = get_object_type(&b);
    c->sample_rate = get_sample_rate(&b, &c->sampling_index);
    c->chan_config = (int)pc_bits(&b, 4);
    c->sbr = -1;
    c->ps = -1;
    if (c->object_type == HEAAC_AOT_SBR ||
        (c->object_type == HEAAC_AOT_PS && !((pc_peek(&b, 3) & 0x03) && !(pc_peek(&b, 9) & 0x3F)))) {
        if (c->object_type == HEAAC_AOT_PS) c->ps = 1;
        c->ext_object_type = HEAAC_AOT_SBR;
        c->sbr = 1;
        c->ext_sample_rate = get_sample_rate(&b, &c->ext_sampling_index);
        c->object_type = get_object_type(&b);
        if (c->object_type == 22)                      /* AOT_ER_BSAC */
            c->ext_chan_config = (int)pc_bits(&b, 4);
    }
    const int specific = b.pos;
    if (c->object_type == 36)                          /* AOT_ALS: not an AAC configuration */
        return HEAAC_PARSE_ERR_UNSUPPORTED;
    if (c->ext_object_type != HEAAC_AOT_SBR) {
        while (pc_left(&b) > 15) {
            if (pc_peek(&b, 11) == 0x2b7) {               /* sync extension */
                pc_bits(&b, 11);
                c->ext_object_type = get_object_type(&b);
                if (c->ext_object_type == HEAAC_AOT_SBR && (c->sbr = (int)pc_bit1(&b)) == 1)
                    c->ext_sample_rate = get_sample_rate(&b, &c->ext_sampling_index);
                if (pc_left(&b) > 11 && pc_bits(&b, 11) == 0x548)
                    c->ps = (int)pc_bit1(&b);
                break;
            }
            pc_bit1(&b);
        }
    }
    if (!c->sbr) c->ps = 0;                            /* PS requires SBR */
    const int channels = c->chan_config < 8 ? (c->chan_config == 7 ? 8 : c->chan_config) : 0;
    if ((c->ps == -1 && c->object_type != HEAAC_AOT_AAC_LC) || (channels & ~0x01))
        c->ps = 0;                                     /* implicit PS only in the HE-AACv2 profile */
    if (b.over) return HEAAC_PARSE_ERR_OVERREAD;
    return specific;
}

/* GASpecificConfig behind the AudioSpecificConfig (decode_ga_specific_config, aacdec.c:401-452): the
 * 960-sample frame length is refused as the reference refuses it; dependsOnCoreCoder / coreCoderDelay and
 * extensionFlag are read past.  channel_config 0 (a program config element follows) is outside this slice. */
int heaac_ga_specific_config(const HeaacAacConfig *c, const uint8_t *buf, int size, int bit_offset)
{
    if (!c || !buf || size <= 0 || bit_offset < 0) return HEAAC_PARSE_ERR_ARG;
    PcBits b;
    pc_init(&b, buf, size);
    pc_skip(&b, bit_offset);
    if (pc_bit1(&b)) return HEAAC_PARSE_ERR_UNSUPPORTED;          /* frameLengthFlag: 960/120 MDCT window */
    if (pc_bit1(&b)) pc_skip(&b, 14);                                /* dependsOnCoreCoder: coreCoderDelay */
    pc_bit1(&b);                                                  /* extensionFlag (no ER object types here) */
    if (c->chan_config == 0) return HEAAC_PARSE_ERR_UNSUPPORTED;
    if (b.over) return HEAAC_PARSE_ERR_OVERREAD;
    return 0;
}

int heaac_adts_parse_header(HeaacAdtsHeader *h, const uint8_t *buf, int size)
{
    if (!h || !buf || size < 7) return HEAAC_PARSE_ERR_ARG;
    PcBits b;
    pc_init(&b, buf, size);
    const int hs = pc_adts_header(&b, h);
    if (hs < 0) return hs;
    h->sample_rate = k_rates[h->sampling_index];
    h->samples = h->num_aac_frames * 1024;
    h->bit_rate = (int)((long long)h->frame_length * 8 * h->sample_rate / h->samples);
    return hs;
}

/* ------------------------------------------------------------------------------------------ */
/* individual channel stream: the readers of parse_core.h, and what the host does on top         */
/* ------------------------------------------------------------------------------------------ */
enum { TYPE_SCE, TYPE_CPE, TYPE_CCE, TYPE_LFE, TYPE_DSE, TYPE_PCE, TYPE_FIL, TYPE_END };

/* A pulse of amplitude `amp` on a line that has already been dequantised and scaled (:1222-1236): the reference
 * goes back to the quantised magnitude through float arithmetic -- x / sf, then x / x^(1/4) = |q| up to rounding --
 * adds the amplitude AWAY from zero (towards minus infinity on an empty line) and raises to 4/3 again as
 * cbrtf(|q|) * q.  All of it in float, in this order. */
static inline float pulse_add(float line, int amp, float sf)
{
    float q = -(float)amp;
    if (line != 0.0f) {
        const float x = line / sf;
        q = x / sqrtf(sqrtf(fabsf(x))) + (x > 0 ? (float)amp : -(float)amp);
    }
    return cbrtf(fabsf(q)) * q * sf;
}

/* the end of decode_spectrum_and_dequant for channel c, once pc_ics has decoded it: the pulses it read into pg */
static void add_pulses(const HeaacToolsChannel *ch, const PcHost *pg, int c, float coef[1024])
{
    if (!pg->decoded[c]) return;
    int band = 0;
    for (int i = 0; i < pg->num_pulse[c]; i++) {
        const int line = pg->pulse_pos[c][i];
        while (ch->ics.swb_offset[band + 1] <= line) band++;
        /* no pulses into noise bands or bands without a scalefactor (:1227) */
        if (ch->band_type[band] == HEAAC_NOISE_BT || ch->sf[band] == 0.0f) continue;
        coef[line] = pulse_add(coef[line], pg->pulse_amp[c][i], ch->sf[band]);
    }
}

/* pc_che as the element loops call it (tools->ch[0] alone for a single channel; *pg zeroed ahead of the element):
 * HEAAC_PARSE_OK or the refusal's status */
static int read_che(const HeaacAacConfig *cfg, const HeaacParseTables *t, PcBits *b, int pair, HeaacToolsFrame *tools,
                    uint32_t w[2], float *coeffs, PcHost *pg)
{
    const int r = pc_che(cfg, t, &t->lut[0][0], b, pair, tools, w, coeffs, pg);
    add_pulses(&tools->ch[0], pg, 0, coeffs);
    if (pair) add_pulses(&tools->ch[1], pg, 1, coeffs + 1024);
    return r ? pg->status : HEAAC_PARSE_OK;
}

/* program_config_element: read past (decode_pce, aacdec.c:303-357).  The reference turns it into a channel
 * layout (output_configure); this slice keeps the layout of the configuration. */
static int skip_pce(PcBits *b)
{
    pc_bits(b, 2);                                        /* object_type */
    pc_bits(b, 4);                                        /* sampling_index */
    const int num_front = (int)pc_bits(b, 4), num_side = (int)pc_bits(b, 4), num_back = (int)pc_bits(b, 4);
    const int num_lfe = (int)pc_bits(b, 2), num_assoc = (int)pc_bits(b, 3), num_cc = (int)pc_bits(b, 4);
    if (pc_bit1(b)) pc_bits(b, 4);                           /* mono_mixdown_tag */
    if (pc_bit1(b)) pc_bits(b, 4);                           /* stereo_mixdown_tag */
    if (pc_bit1(b)) pc_bits(b, 3);                           /* mixdown_coeff_index, pseudo_surround */
    pc_skip(b, 5 * (num_front + num_side + num_back));    /* is_cpe + tag per element */
    pc_skip(b, 4 * num_lfe);
    pc_skip(b, 4 * num_assoc);
    pc_skip(b, 5 * num_cc);                               /* cc_element_is_ind_sw + tag */
    b->pos = (b->pos + 7) & ~7;
    const int comment = 8 * (int)pc_bits(b, 8);
    if (pc_left(b) < comment) return HEAAC_PARSE_ERR_OVERREAD;
    pc_skip(b, comment);
    return HEAAC_PARSE_OK;
}

/* coupling_channel_element (decode_cce, aacdec.c:1503-1570) */
typedef struct { int type, id, ch_select; } CceTarget;
/* A coupling element as transmitted: its target list and its gain lists in transmission order (:1538-1567).  Which
 * of the lists land on an output element is cce_resolve's. */
typedef struct {
    int num_coupled;
    CceTarget tg[8];
    float gl[16][120];
} CceLists;

/* One coupling gain.  The reference keeps the base in a `float scale` (aacdec.c:1508, :1528: 2^(1/8), 2^(1/4), 2^(1/2)
 * are ROUNDED to float before anything is raised to a power), calls the double pow() on it and rounds the result to
 * float (:1539, :1556; the sign is applied in double, which is exact). */
static float cce_gain(float base, int step, int negative)
{
    const double mag = pow((double)base, (double)-step);
    return (float)(negative ? -mag : mag);
}

/* The target list (:1511-1523).  Returns the number of gain lists that follow the channel stream: one per target,
 * two for a pair coupled with a gain list per channel. */
static int cce_read_targets(PcBits *b, CceLists *ls)
{
    int lists = 0;
    ls->num_coupled = (int)pc_bits(b, 3);
    for (int c = 0; c <= ls->num_coupled; c++) {
        CceTarget *t = &ls->tg[c];
        const int pair = (int)pc_bit1(b);
        t->type = pair ? TYPE_CPE : TYPE_SCE;
        t->id = (int)pc_bits(b, 4);
        t->ch_select = pair ? (int)pc_bits(b, 2) : 2;
        lists += 1 + (t->ch_select == 3);
    }
    return lists;
}

/* How one gain list is coded. */
typedef struct {
    float base;            /* gain_element_scale as the reference's float */
    int sign_coded;        /* gain_element_sign: the low bit of an accumulated step is the sign */
    int common;            /* one gain for the whole list (always, for the first list: gain 1) */
    int first;             /* the first list carries no common gain: it starts from 1.0f */
} CceListCoding;

/* One gain list over the coupling channel's scalefactor bands (:1534-1566).  A list with a common gain holds that
 * value in every coded band; otherwise each coded band transmits a step that ACCUMULATES (`t = gain += t`), a zero
 * step repeating the value before it -- which, before the first non-zero step, is the list's starting value. */
static int cce_read_gain_list(const HeaacParseTables *t, PcBits *b, const CceListCoding *k, const HeaacToolsChannel *ch, int after_imdct,
                              float out[120])
{
    int acc = 0;
    float cur = 1.0f;
    if (!k->first) {
        if (k->common) {
            const int sym = pc_tree(t, &t->lut[0][0], 0, b);
            if (sym < 0) return HEAAC_PARSE_ERR_DATA;
            acc = sym - 60;
        }
        cur = cce_gain(k->base, acc, 0);               /* unsigned whatever gain_element_sign says (:1539) */
    }
    if (after_imdct) {
        out[0] = cur;
        return HEAAC_PARSE_OK;
    }
    const int n_bands = ch->ics.num_window_groups * ch->ics.max_sfb;
    if (n_bands > 120) return HEAAC_PARSE_ERR_DATA;
    for (int band = 0; band < n_bands; band++) {
        if (ch->band_type[band] == 0) continue;        /* ZERO_BT: no gain, no bits */
        if (!k->common) {
            const int sym = pc_tree(t, &t->lut[0][0], 0, b);
            if (sym < 0) return HEAAC_PARSE_ERR_DATA;
            if (sym != 60) {
                acc += sym - 60;
                /* arithmetic shift of the accumulated step, the low bit being the sign (:1552-1555) */
                cur = k->sign_coded ? cce_gain(k->base, acc >> 1, acc & 1) : cce_gain(k->base, acc, 0);
            }
        }
        out[band] = cur;
    }
    return HEAAC_PARSE_OK;
}

static int read_cce(const HeaacAacConfig *cfg, const HeaacParseTables *t, PcBits *b, int elem_id, HeaacCceFrame *out, CceLists *ls,
                    HeaacToolsFrame *tools, uint32_t *w, float coef[1024])
{
    const HeaacToolsChannel *ch = &tools->ch[0];    /* the coupling channel */
    memset(out, 0, sizeof(*out));
    out->present = 1;
    out->elem_id = (uint8_t)elem_id;
    const int independent = (int)pc_bit1(b);              /* ind_sw_cce_flag */
    const int n_lists = cce_read_targets(b, ls);
    const int after_tns = (int)pc_bit1(b);                /* cc_domain; read either way (:1524) */
    const int point = independent ? HEAAC_CC_AFTER_IMDCT : after_tns;
    out->coupling_point = (uint8_t)point;
    CceListCoding k;
    k.sign_coded = (int)pc_bit1(b);
    k.base = (float)pow(2., pow(2., (int)pc_bits(b, 2) - 3));
    PcHost pg;                                         /* a refusal inside a coupling element is not followed up */
    memset(&pg, 0, sizeof(pg));
    int r = read_che(cfg, t, b, 0, tools, w, coef, &pg);
    if (r < 0) return r;
    out->ics = ch->ics;
    memcpy(out->band_type, ch->band_type, sizeof(out->band_type));

    memset(ls->gl, 0, sizeof(ls->gl));
    for (int c = 0; c < n_lists; c++) {
        k.first = c == 0;
        k.common = k.first || point == HEAAC_CC_AFTER_IMDCT || pc_bit1(b);
        if ((r = cce_read_gain_list(t, b, &k, ch, point == HEAAC_CC_AFTER_IMDCT, ls->gl[c])) < 0) return r;
    }
    return HEAAC_PARSE_OK;
}

/* Which lists land on the output element (target_type, target_id), and on which of its channels: the index walk of
 * apply_channel_coupling (:1870-1898) -- every entry of the target list consumes one gain list, or two for a pair
 * coupled with separate gains (ch_select 3), whether or not it names this element. */
static int cce_resolve(const CceLists *ls, int target_type, int target_id, HeaacCceFrame *out)
{
    int index = 0, n_links = 0;
    for (int c = 0; c <= ls->num_coupled; c++) {
        const CceTarget *tg = &ls->tg[c];
        if (tg->type == target_type && tg->id == target_id) {
            int use[2], nuse = 0, chn[2];
            if (tg->ch_select != 1) {
                use[nuse] = index; chn[nuse++] = 0;
                if (tg->ch_select != 0) index++;
            }
            if (tg->ch_select != 2) { use[nuse] = index++; chn[nuse++] = 1; }
            for (int k = 0; k < nuse; k++) {
                if (n_links >= HEAAC_MAX_CCE_LINKS) return HEAAC_PARSE_ERR_UNSUPPORTED;
                out->link[n_links].target_ch = (uint8_t)chn[k];
                memcpy(out->link[n_links].gain, ls->gl[use[k]], sizeof(out->link[n_links].gain));
                n_links++;
            }
        } else {
            index += 1 + (tg->ch_select == 3);
        }
    }
    out->n_links = (uint8_t)n_links;
    return HEAAC_PARSE_OK;
}

int heaac_aac_parse_frame(const HeaacAacConfig *cfg, HeaacAacStream *st,
                          const uint8_t *au, int size,
                          float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                          HeaacAacFrameInfo *info)
{
    return heaac_aac_parse_frame_ex(cfg, st, au, size, 2, coeffs, ics, tools, NULL, info);
}

/* a refusal of the element loops' own, recorded as the readers of parse_core.h record theirs */
#define REF_FAIL(pg, code) (pc_refuse(pg, code, 1), (code))
#define REF_OVERREAD(pg) (pc_refuse(pg, HEAAC_PARSE_ERR_OVERREAD, 2), HEAAC_PARSE_ERR_OVERREAD)

/* The walk over one access unit of a one-element stream; `b`, `w`, `pg`, `n_cce_seen` are the caller's so that it
 * can tell, after a refusal, how far the walk had got. */
static int frame_walk(const HeaacAacConfig *cfg, HeaacAacStream *st, const uint8_t *au, int size, int coeff_channels,
                      float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools, const HeaacCceOut *cce,
                      HeaacAacFrameInfo *info, const HeaacParseTables *t, PcBits *b, uint32_t w[2], PcHost *pg, int *n_cce_seen)
{
    pc_init(b, au, size);
    /* st->mapped_tag and st->oc are kept whatever becomes of the unit, as tag_che_map and the output configuration are */
    if (pc_peek(b, 12) == 0xfff && pc_adts(cfg, b, &st->mapped_tag, &st->oc, pg)) return pg->status;
    uint32_t wc[HEAAC_MAX_CCE];
    for (int c = 0; c < 2; c++) w[c] = pc_win_load(st->window_sequence[c], st->use_kb_window[c]);
    HeaacAacFrameInfo fi = { 0, 0, -1, 0, 0, 0, 0, 0, 0 };
    int last_che = 0, prev_type = TYPE_END;            /* 1 + type of the channel element last seen; the element in front */
    /* The coupling elements name their targets by (type, tag): the output element of this slice is the one SCE /
     * CPE of the configuration (set_default_channel_config: tag 0), known before the walk starts. */
    const int target_type = cfg->chan_config == 2 ? TYPE_CPE : TYPE_SCE;
    int cce_tag[HEAAC_MAX_CCE], n_cce = 0;
    if (cce) memset(cce->cce, 0, HEAAC_MAX_CCE * sizeof(HeaacCceFrame));
    int elem, r;
    while ((elem = (int)pc_bits(b, 3)) != TYPE_END) {
        const int elem_id = (int)pc_bits(b, 4);
        switch (elem) {
        case TYPE_SCE:
        case TYPE_CPE:
            if (pc_output_element(cfg, &st->mapped_tag, elem, elem_id, fi.channels, pg)) return pg->status;
            if (elem == TYPE_CPE && coeff_channels < 2) return HEAAC_PARSE_ERR_ARG;
            if ((r = read_che(cfg, t, b, elem == TYPE_CPE, tools, w, coeffs, pg)) < 0) return r;
            fi.channels = elem + 1;
            fi.elem_id = elem_id;
            break;
        case TYPE_CCE: {
            if (!cce || n_cce >= HEAAC_MAX_CCE) return HEAAC_PARSE_ERR_UNSUPPORTED;
            for (int k = 0; k < n_cce; k++)
                if (cce_tag[k] == elem_id) return HEAAC_PARSE_ERR_DATA;           /* the same element twice */
            /* slots in ascending tag order: a smaller tag arriving later moves the earlier element up */
            int slot = n_cce;
            while (slot > 0 && cce_tag[slot - 1] > elem_id) {
                cce->cce[slot] = cce->cce[slot - 1];
                cce->tools[slot] = cce->tools[slot - 1];
                memcpy(cce->coeffs + slot * 1024, cce->coeffs + (slot - 1) * 1024, 4096);
                wc[slot] = wc[slot - 1];
                cce_tag[slot] = cce_tag[slot - 1];
                slot--;
            }
            cce_tag[slot] = elem_id;
            n_cce++;
            *n_cce_seen = n_cce;
            /* the coupling channel's window history: by instance tag, as the reference keeps it (che[TYPE_CCE][tag]) --
             * slots move with the tags an access unit happens to carry and the order they arrive in */
            wc[slot] = pc_win_load(st->cce_window_sequence[elem_id], st->cce_use_kb_window[elem_id]);
            memset(&cce->tools[slot], 0, sizeof(HeaacToolsFrame));
            CceLists ls;
            r = read_cce(cfg, t, b, elem_id, &cce->cce[slot], &ls, &cce->tools[slot], &wc[slot],
                         cce->coeffs + slot * 1024);
            if (r < 0) return r;
            if ((r = cce_resolve(&ls, target_type, 0, &cce->cce[slot])) < 0) return r;
            cce->cce[slot].behind_target = cce->cce[slot].outputs_before = (uint8_t)(fi.channels != 0);
            cce->cce[slot].seq = (uint8_t)(n_cce - 1);
            break;
        }
        case TYPE_LFE:
            /* no LFE in a one- or two-channel layout: get_che finds no element for it ("channel element %d.%d is not
             * allocated", :2011-2015) */
            return REF_FAIL(pg, HEAAC_PARSE_ERR_UNSUPPORTED);
        case TYPE_DSE:
            if (pc_dse(b, pg)) return pg->status;
            break;
        case TYPE_PCE:
            if ((r = skip_pce(b)) < 0) return r;
            break;
        case TYPE_FIL: {
            /* an SBR payload is located here and parsed by sbr_parse.c.  decode_extension_payload hands it to the
             * channel element last seen, together with the type of the element directly in front (:2059) */
            int at, bytes = 0, crc = 0;
            if (pc_fil(b, elem_id, &at, &bytes, &crc, pg)) return pg->status;
            if (at >= 0) {
                if (!last_che) return HEAAC_PARSE_ERR_DATA;            /* "SBR was found before the first channel element" */
                if (last_che == TYPE_CCE + 1) return HEAAC_PARSE_ERR_UNSUPPORTED;   /* the coupling element's own SBR */
                if (fi.sbr_payload_bit >= 0) return HEAAC_PARSE_ERR_UNSUPPORTED;    /* a second payload for the element */
                fi.sbr_payload_bit = at;
                fi.sbr_payload_bytes = bytes;
                fi.sbr_crc = crc;
                fi.sbr_misplaced = prev_type != TYPE_SCE && prev_type != TYPE_CPE;
                pc_implicit_ps(cfg, &st->mapped_tag, &st->oc);
            }
            break;
        }
        default:
            return HEAAC_PARSE_ERR_UNSUPPORTED;
        }
        if (elem < TYPE_DSE) last_che = elem + 1;
        prev_type = elem;
        if (b->over) return HEAAC_PARSE_ERR_OVERREAD;
        if (pc_left(b) < 3) return REF_OVERREAD(pg);                             /* :2072-2075 */
    }
    if (!fi.channels) return HEAAC_PARSE_ERR_DATA;
    if (fi.elem_id != 0 && n_cce) {
        /* the links were resolved against tag 0 (the default layout's): an output element with another tag is only
         * reachable through a program config element */
        return HEAAC_PARSE_ERR_UNSUPPORTED;
    }
    for (int c = 0; c < fi.channels; c++) pc_win_store(w[c], &ics[c], &st->window_sequence[c], &st->use_kb_window[c]);
    for (int k = 0; k < n_cce; k++)
        pc_win_store(wc[k], &cce->ics[k], &st->cce_window_sequence[cce_tag[k]], &st->cce_use_kb_window[cce_tag[k]]);
    fi.n_cce = n_cce;
    fi.bits_consumed = b->pos;
    if (info) *info = fi;
    return HEAAC_PARSE_OK;
}

/* A channel record that only draws `draws` numbers from the noise generator (bands of at most 96 lines, the widest
 * the band tables have) and leaves the predictors alone: one long window, so that no reset applies. */
static void noise_only_channel(HeaacToolsChannel *ch, float *coef, int draws)
{
    memset(ch, 0, sizeof(*ch));
    if (coef) memset(coef, 0, 1024 * sizeof(float));
    ch->ics.num_windows = ch->ics.num_window_groups = ch->ics.group_len[0] = 1;
    int nb = 0, at = 0;
    while (draws > 0) {
        const int len = draws < 96 ? draws : 96;
        ch->ics.swb_offset[nb] = (uint16_t)at;
        ch->band_type[nb] = HEAAC_NOISE_BT;
        ch->sf[nb] = 1.0f;
        at += len;
        draws -= len;
        nb++;
    }
    ch->ics.swb_offset[nb] = (uint16_t)at;
    ch->ics.max_sfb = ch->ics.num_swb = (uint8_t)nb;
}

/* The noise bands among the first `stop` bands of a channel, in lines (= numbers drawn, :1016-1029) */
static int noise_draws(const HeaacToolsChannel *ch, int stop)
{
    int idx = 0, draws = 0;
    for (int g = 0; g < ch->ics.num_window_groups; g++)
        for (int i = 0; i < ch->ics.max_sfb; i++, idx++)
            if (idx < stop && ch->band_type[idx] == HEAAC_NOISE_BT)
                draws += ch->ics.group_len[g] * (ch->ics.swb_offset[i + 1] - ch->ics.swb_offset[i]);
    return draws;
}

/* A refused access unit gives no samples, but what the reference's element decoders did before they gave up is not
 * undone (aac_decode_frame returns from the middle of its element loop, :2069-2070): the window history that
 * decode_ics_info moved on or cleared, the numbers decode_spectrum_and_dequant drew for the noise bands it had passed,
 * the predictors apply_prediction stepped for a channel it completed.  Where the refusal is the reference's own,
 * `st` takes the same history here, and `tools` / `coeffs` are rewritten into records that make the spectral tools
 * draw and predict exactly that much (HEAAC_REFUSED_RUN_TOOLS); their coefficients are of no further use. */
static void unit_refused(const HeaacAacConfig *cfg, HeaacAacStream *st, const PcBits *b, const uint32_t w[2],
                         const PcHost *pg, int n_cce, int coeff_channels, float *coeffs, HeaacToolsFrame *tools,
                         HeaacAacFrameInfo *info)
{
    HeaacAacFrameInfo fi = { 0, 0, -1, 0, 0, 0, 0, 0, 0 };
    if (pg->as_reference && (!b->over || pg->ref_overread) && !n_cce) {
        fi.refused = HEAAC_REFUSED_AS_REFERENCE;
        for (int c = 0; c < 2; c++) {
            if (pg->ics[c] == 1) {
                st->window_sequence[c] = (uint8_t)PC_WS0(w[c]);
                st->use_kb_window[c] = (uint8_t)PC_KB0(w[c]);
            } else if (pg->ics[c] == 2) {
                st->window_sequence[c] = st->use_kb_window[c] = 0;
            }
        }
        const int main_profile = cfg->object_type == HEAAC_AOT_AAC_MAIN;
        const int complete = pg->decoded[0] && (pg->ics[1] == 0 || pg->decoded[1]) &&
                             (!main_profile || (pg->predicted[0] && (pg->ics[1] == 0 || pg->predicted[1])));
        int work = 0;
        if (complete) {
            /* the element was decoded to its end (the refusal came behind it): its records stand as they are */
            work = main_profile || noise_draws(&tools->ch[0], 128) || (pg->ics[1] && noise_draws(&tools->ch[1], 128));
        } else {
            tools->common_window = tools->ms_present = 0;
            memset(tools->ms_mask, 0, sizeof(tools->ms_mask));
            for (int c = 0; c < 2; c++) {
                HeaacToolsChannel *ch = &tools->ch[c];
                float *coef = c < coeff_channels ? coeffs + c * 1024 : NULL;
                if (pg->decoded[c] && (!main_profile || pg->predicted[c])) {
                    work |= main_profile || noise_draws(ch, 128);
                    memset(&ch->tns, 0, sizeof(ch->tns));
                } else {
                    /* a channel that stopped inside its spectrum, or one whose prediction was still to come at the
                     * end of the pair: only its noise bands have left a trace */
                    const int draws = pg->ics[c] == 1 ? noise_draws(ch, pg->decoded[c] ? 128 : pg->noise_stop[c]) : 0;
                    noise_only_channel(ch, coef, draws);
                    work |= draws;
                }
            }
        }
        if (work) fi.refused |= HEAAC_REFUSED_RUN_TOOLS;
    }
    if (info) *info = fi;
}

int heaac_aac_parse_frame_ex(const HeaacAacConfig *cfg, HeaacAacStream *st,
                             const uint8_t *au, int size, int coeff_channels,
                             float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                             const HeaacCceOut *cce, HeaacAacFrameInfo *info)
{
    if (!cfg || !st || !au || size <= 0 || !coeffs || !ics || !tools ||
        cfg->sampling_index < 0 || cfg->sampling_index > 12 || coeff_channels < 1 || coeff_channels > 2 ||
        (cce && (!cce->cce || !cce->coeffs || !cce->ics || !cce->tools)))
        return HEAAC_PARSE_ERR_ARG;
    const HeaacParseTables *t = heaac_parse_tables();
    if (!t) return HEAAC_PARSE_ERR_ARG;
    PcBits b;
    uint32_t w[2];
    PcHost pg;
    int n_cce = 0;
    memset(&pg, 0, sizeof(pg));
    memset(w, 0, sizeof(w));
    memset(tools, 0, sizeof(*tools));
    const int r = frame_walk(cfg, st, au, size, coeff_channels, coeffs, ics, tools, cce, info, t, &b, w, &pg, &n_cce);
    if (r < 0) unit_refused(cfg, st, &b, w, &pg, n_cce, coeff_channels, coeffs, tools, info);
    else if (!(st->oc & PC_OC_NONE)) st->oc |= PC_OC_LOCKED;     /* the unit decodes: output_configured = OC_LOCKED */
    return r;
}

/* ------------------------------------------------------------------------------------------ */
/* channel layouts: several output elements per access unit                                      */
/* ------------------------------------------------------------------------------------------ */
typedef struct { uint8_t type, id; } ElemRef;
/* The channel configurations 1..7 twice: the order the elements' channels leave the decoder
 * (aac_channel_layout_map, aacdectab.h:74-82) and the order the elements arrive in an access unit, which is what
 * get_che maps by (:138-181: the n-th output element of the stream must have the type standing here; where a
 * 5.1 / 7.1 layout has its LFE an SCE is taken too).  Mask = aac_channel_layout[] (aacdectab.h:84-93). */
static const struct ChanConfig {
    int n;
    ElemRef out[5], arrive[5];
    int64_t mask;
} k_chan_config[8] = {
    { 0, {{0, 0}}, {{0, 0}}, 0 },
    { 1, {{TYPE_SCE, 0}},                                                        {{TYPE_SCE, 0}}, 0x4 },
    { 1, {{TYPE_CPE, 0}},                                                        {{TYPE_CPE, 0}}, 0x3 },
    { 2, {{TYPE_CPE, 0}, {TYPE_SCE, 0}},                                         {{TYPE_SCE, 0}, {TYPE_CPE, 0}}, 0x7 },
    { 3, {{TYPE_CPE, 0}, {TYPE_SCE, 0}, {TYPE_SCE, 1}},                          {{TYPE_SCE, 0}, {TYPE_CPE, 0}, {TYPE_SCE, 1}}, 0x107 },
    { 3, {{TYPE_CPE, 0}, {TYPE_SCE, 0}, {TYPE_CPE, 1}},                          {{TYPE_SCE, 0}, {TYPE_CPE, 0}, {TYPE_CPE, 1}}, 0x37 },
    { 4, {{TYPE_CPE, 0}, {TYPE_SCE, 0}, {TYPE_LFE, 0}, {TYPE_CPE, 1}},           {{TYPE_SCE, 0}, {TYPE_CPE, 0}, {TYPE_CPE, 1}, {TYPE_LFE, 0}}, 0x3f },
    { 5, {{TYPE_CPE, 0}, {TYPE_SCE, 0}, {TYPE_LFE, 0}, {TYPE_CPE, 2}, {TYPE_CPE, 1}},
         {{TYPE_SCE, 0}, {TYPE_CPE, 0}, {TYPE_CPE, 1}, {TYPE_CPE, 2}, {TYPE_LFE, 0}}, 0xff },
};

static int layout_add(HeaacAacLayout *l, int type, int id)
{
    const int nch = type == TYPE_CPE ? 2 : 1;
    if (l->n_elements >= HEAAC_MAX_ELEMENTS || l->channels + nch > HEAAC_MAX_LAYOUT_CHANNELS) return HEAAC_PARSE_ERR_UNSUPPORTED;
    HeaacAacElementSlot *e = &l->elem[l->n_elements];
    e->type = (uint8_t)type; e->id = (uint8_t)id; e->channels = (uint8_t)nch; e->first_channel = (uint8_t)l->channels;
    l->slot_of[type][id] = (int8_t)(l->n_elements + 1);
    l->n_elements++;
    l->channels += nch;
    return 0;
}

int heaac_aac_layout_default(HeaacAacLayout *l, int chan_config)
{
    if (!l) return HEAAC_PARSE_ERR_ARG;
    memset(l, 0, sizeof(*l));
    if (chan_config < 1 || chan_config > 7) return HEAAC_PARSE_ERR_DATA;   /* "invalid default channel configuration" */
    const struct ChanConfig *c = &k_chan_config[chan_config];
    l->chan_config = chan_config;
    for (int i = 0; i < c->n; i++) layout_add(l, c->out[i].type, c->out[i].id);
    l->channel_layout = c->mask;
    return 0;
}

int heaac_aac_layout_from_pce(HeaacAacLayout *l, const uint8_t *buf, int size, int bit_offset, int *bits_used)
{
    if (!l || !buf || size <= 0 || bit_offset < 0) return HEAAC_PARSE_ERR_ARG;
    PcBits b;
    pc_init(&b, buf, size);
    pc_skip(&b, bit_offset);
    uint8_t have[4][16];
    memset(have, 0, sizeof(have));
    pc_bits(&b, 2);                                       /* object_type */
    pc_bits(&b, 4);                                       /* sampling_index (a mismatch with the configuration only warns) */
    const int num[3] = { (int)pc_bits(&b, 4), (int)pc_bits(&b, 4), (int)pc_bits(&b, 4) };   /* front, side, back */
    const int num_lfe = (int)pc_bits(&b, 2), num_assoc = (int)pc_bits(&b, 3), num_cc = (int)pc_bits(&b, 4);
    if (pc_bit1(&b)) pc_bits(&b, 4);                         /* mono_mixdown_tag */
    if (pc_bit1(&b)) pc_bits(&b, 4);                         /* stereo_mixdown_tag */
    if (pc_bit1(&b)) pc_bits(&b, 3);                         /* mixdown_coeff_index, pseudo_surround */
    for (int g = 0; g < 3; g++)
        for (int i = 0; i < num[g]; i++) {
            const int pair = (int)pc_bit1(&b);
            have[pair ? TYPE_CPE : TYPE_SCE][pc_bits(&b, 4)] = 1;
        }
    for (int i = 0; i < num_lfe; i++) have[TYPE_LFE][pc_bits(&b, 4)] = 1;
    pc_skip(&b, 4 * num_assoc);
    for (int i = 0; i < num_cc; i++) {
        pc_bit1(&b);                                      /* cc_element_is_ind_sw: the element says so itself */
        have[TYPE_CCE][pc_bits(&b, 4)] = 1;
    }
    b.pos = (b.pos + 7) & ~7;
    const int comment = 8 * (int)pc_bits(&b, 8);
    if (b.over || pc_left(&b) < comment) return HEAAC_PARSE_ERR_OVERREAD;
    pc_skip(&b, comment);
    memset(l, 0, sizeof(*l));
    /* output_configure without a channel configuration (:253-268): ids ascending, per id SCE, CPE, (CCE,) LFE */
    for (int id = 0; id < 16; id++) {
        static const int order[3] = { TYPE_SCE, TYPE_CPE, TYPE_LFE };
        for (int t = 0; t < 3; t++)
            if (have[order[t]][id] && layout_add(l, order[t], id) < 0) return HEAAC_PARSE_ERR_UNSUPPORTED;
    }
    /* the coupling elements the program names (che_configure allocates no others, :198-212): not output elements;
     * their slots, in ascending tag order, are the order apply_channel_coupling walks them in (:1876) */
    for (int id = 0, k = 0; id < 16; id++)
        if (have[TYPE_CCE][id]) l->slot_of[TYPE_CCE][id] = (int8_t)++k;
    memcpy(l->tag_map, l->slot_of, sizeof(l->tag_map));      /* tag_che_map = che: elements are found by their tag */
    l->tags_mapped = 4 * 16;
    if (bits_used) *bits_used = b.pos - bit_offset;
    return 0;
}

int heaac_aac_layout_from_au(HeaacAacLayout *l, const uint8_t *au, int size)
{
    if (!l || !au || size <= 0) return HEAAC_PARSE_ERR_ARG;
    PcBits b;
    pc_init(&b, au, size);
    if (pc_peek(&b, 12) == 0xfff) {
        HeaacAdtsHeader h;
        const int hs = heaac_adts_parse_header(&h, au, size);
        if (hs < 0) return HEAAC_PARSE_ERR_DATA;
        b.pos = hs * 8;
    }
    /* aac_decode_frame's element loop (:1999-2075) as far as the first program config element: with nothing allocated
     * yet only data stream and fill elements can stand in front of it */
    int type;
    while ((type = (int)pc_bits(&b, 3)) != TYPE_END) {
        const int tag = (int)pc_bits(&b, 4);
        if (type == TYPE_PCE) {
            if (b.over) return HEAAC_PARSE_ERR_OVERREAD;
            return heaac_aac_layout_from_pce(l, au, size, b.pos, NULL);
        }
        if (type == TYPE_DSE) {
            if (pc_dse(&b, NULL)) return HEAAC_PARSE_ERR_OVERREAD;
        } else if (type == TYPE_FIL) {
            int at, bytes, crc;
            if (pc_fil(&b, tag, &at, &bytes, &crc, NULL)) return HEAAC_PARSE_ERR_OVERREAD;
            if (at >= 0) return HEAAC_PARSE_ERR_DATA;                  /* "SBR was found before the first channel element" */
        } else {
            return HEAAC_PARSE_ERR_DATA;                               /* "channel element %d.%d is not allocated" */
        }
        if (b.over || pc_left(&b) < 3) return HEAAC_PARSE_ERR_OVERREAD;
    }
    return HEAAC_PARSE_ERR_DATA;                                       /* no program: nothing this stream could decode */
}

int heaac_asc_layout(HeaacAacConfig *c, HeaacAacLayout *l, const uint8_t *buf, int size)
{
    if (!c || !l) return HEAAC_PARSE_ERR_ARG;
    const int specific = heaac_asc_parse(c, buf, size);
    if (specific < 0) return specific;
    /* decode_ga_specific_config (:401-452) */
    PcBits b;
    pc_init(&b, buf, size);
    pc_skip(&b, specific);
    if (pc_bit1(&b)) return HEAAC_PARSE_ERR_UNSUPPORTED;          /* frameLengthFlag: 960/120 MDCT window */
    if (pc_bit1(&b)) pc_skip(&b, 14);                                /* dependsOnCoreCoder: coreCoderDelay */
    pc_bit1(&b);                                                  /* extensionFlag (no ER object types here) */
    if (b.over) return HEAAC_PARSE_ERR_OVERREAD;
    if (c->chan_config) return heaac_aac_layout_default(l, c->chan_config);
    pc_skip(&b, 4);                                               /* element_instance_tag of the program config element */
    if (b.over) return HEAAC_PARSE_ERR_OVERREAD;
    return heaac_aac_layout_from_pce(l, buf, size, b.pos, NULL);
}

/* get_che (:113-183): the slot of the layout a bitstream element (type, tag) lands in, or -1 */
static int layout_find(HeaacAacLayout *l, uint8_t seen[4][16], int type, int *tag_io)
{
    int tag = *tag_io;
    /* "Some buggy encoders appear to set all elem_ids to zero": a tag met twice in one access unit moves up */
    while (tag < 16 && seen[type][tag]) tag++;
    if (tag == 16) return -1;
    seen[type][tag] = 1;
    *tag_io = tag;
    if (l->tag_map[type][tag]) return l->tag_map[type][tag] - 1;
    if (l->chan_config < 1 || l->chan_config > 7) return -1;
    const struct ChanConfig *c = &k_chan_config[l->chan_config];
    if (l->tags_mapped >= c->n) return -1;
    const ElemRef want = c->arrive[l->tags_mapped];
    if (type != want.type && !(want.type == TYPE_LFE && type == TYPE_SCE)) return -1;
    const int slot = l->slot_of[want.type][want.id] - 1;
    l->tag_map[type][tag] = (int8_t)(slot + 1);
    l->tags_mapped++;
    return slot;
}

int heaac_aac_parse_frame_layout(const HeaacAacConfig *cfg, HeaacAacLayout *layout, HeaacAacStream *st,
                                 const uint8_t *au, int size,
                                 float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                                 HeaacAacElementInfo *elem, HeaacAacFrameInfo *info)
{
    return heaac_aac_parse_frame_layout_ex(cfg, layout, st, au, size, coeffs, ics, tools, elem, NULL, info);
}

/* What the walk over a layout's access unit leaves for the caller to judge a refusal by (unit_refused above, per
 * element): the window histories in work, the progress of every element that was completed, of the one the refusal
 * stands in, and of the loop around them. */
typedef struct {
    PcBits b;
    uint32_t w[HEAAC_MAX_ELEMENTS][2];
    PcHost done[HEAAC_MAX_ELEMENTS], at, loop;
    int at_slot, n_cce;
} LayoutWalk;

static int layout_walk(const HeaacAacConfig *cfg, HeaacAacLayout *layout, HeaacAacStream *st, const uint8_t *au, int size,
                       float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools, HeaacAacElementInfo *elem,
                       const HeaacCceOut *cce, HeaacAacFrameInfo *info, const HeaacParseTables *pt, LayoutWalk *lw)
{
    PcBits *b = &lw->b;
    pc_init(b, au, size);
    if (pc_peek(b, 12) == 0xfff && pc_adts(cfg, b, NULL, NULL, &lw->loop)) return lw->loop.status;
    const int ne = layout->n_elements;
    uint32_t (*w)[2] = lw->w;
    for (int e = 0; e < ne; e++)
        for (int c = 0; c < 2; c++) w[e][c] = pc_win_load(st[e].window_sequence[c], st[e].use_kb_window[c]);
    memset(elem, 0, (size_t)ne * sizeof(*elem));
    for (int e = 0; e < ne; e++) elem[e].sbr_payload_bit = -1;
    uint8_t seen[4][16];
    memset(seen, 0, sizeof(seen));
    int n_seen = 0, prev_slot = -1, last_cce = -1, prev_type = TYPE_END, type, r;      /* last_cce: the channel element last seen is coupling slot k */
    /* coupling elements: slot k of the layout's list; lists[k] until the output elements are all known */
    uint32_t wc[HEAAC_MAX_CCE];
    HeaacCceFrame cbase[HEAAC_MAX_CCE];
    CceLists lists[HEAAC_MAX_CCE];
    int n_cce = 0;
    memset(cbase, 0, sizeof(cbase));
    if (cce) memset(cce->cce, 0, (size_t)ne * HEAAC_MAX_CCE * sizeof(HeaacCceFrame));
    if (cce && cce->elem) {
        memset(cce->elem, 0, HEAAC_MAX_CCE * sizeof(*cce->elem));
        for (int k = 0; k < HEAAC_MAX_CCE; k++) cce->elem[k].sbr_payload_bit = -1;
    }
    while ((type = (int)pc_bits(b, 3)) != TYPE_END) {
        int tag = (int)pc_bits(b, 4);
        int slot = -1;
        switch (type) {
        case TYPE_SCE:
        case TYPE_CPE:
        case TYPE_LFE: {
            slot = layout_find(layout, seen, type, &tag);
            if (slot < 0) return REF_FAIL(&lw->loop, HEAAC_PARSE_ERR_DATA);    /* "channel element %d.%d is not allocated" */
            if (slot >= ne) return HEAAC_PARSE_ERR_ARG;                /* a layout record not made by the layout functions */
            /* the element decodes as what the bitstream says it is; a pair needs a pair's slot */
            if ((type == TYPE_CPE) != (layout->elem[slot].channels == 2)) return HEAAC_PARSE_ERR_DATA;
            HeaacToolsFrame *t = &tools[slot];
            memset(t, 0, sizeof(*t));
            float *co = coeffs + (size_t)slot * 2048;
            elem[slot].type = (uint8_t)type;
            elem[slot].tag = (uint8_t)tag;
            elem[slot].seq = (uint8_t)n_seen;
            lw->at_slot = slot;                        /* the element a refusal from here on stands in */
            memset(&lw->at, 0, sizeof(lw->at));
            if ((r = read_che(cfg, pt, b, type == TYPE_CPE, t, w[slot], co, &lw->at)) < 0) return r;
            lw->done[slot] = lw->at;
            lw->at_slot = -1;
            elem[slot].present = 1;
            n_seen++;
            break;
        }
        case TYPE_CCE: {
            /* get_che: a tag met twice moves up; only what a program config element named is allocated */
            while (tag < 16 && seen[TYPE_CCE][tag]) tag++;
            if (tag == 16) return HEAAC_PARSE_ERR_DATA;
            seen[TYPE_CCE][tag] = 1;
            const int k = layout->tag_map[TYPE_CCE][tag] - 1;
            if (k < 0) return REF_FAIL(&lw->loop, HEAAC_PARSE_ERR_DATA);       /* "channel element 2.%d is not allocated" */
            if (!cce || k >= HEAAC_MAX_CCE) return HEAAC_PARSE_ERR_UNSUPPORTED;
            wc[k] = pc_win_load(st[0].cce_window_sequence[tag], st[0].cce_use_kb_window[tag]);
            memset(&cce->tools[k], 0, sizeof(HeaacToolsFrame));
            r = read_cce(cfg, pt, b, tag, &cbase[k], &lists[k], &cce->tools[k], &wc[k], cce->coeffs + k * 1024);
            if (r < 0) return r;
            cbase[k].outputs_before = (uint8_t)n_seen;
            cbase[k].seq = (uint8_t)n_cce++;
            lw->n_cce = n_cce;
            last_cce = k;
            if (cce->elem) {
                cce->elem[k].present = 1;
                cce->elem[k].type = TYPE_CCE;
                cce->elem[k].tag = (uint8_t)tag;
                cce->elem[k].seq = cbase[k].seq;
            }
            break;
        }
        case TYPE_DSE:
            if (pc_dse(b, &lw->loop)) return lw->loop.status;
            break;
        case TYPE_PCE:
            if ((r = skip_pce(b)) < 0) return r;
            break;
        case TYPE_FIL: {
            int at, bytes = 0, crc = 0;
            if (pc_fil(b, tag, &at, &bytes, &crc, &lw->loop)) return lw->loop.status;
            if (at >= 0) {
                /* decode_extension_payload (:1650-1690) hands the payload to the channel element last seen, and to its
                 * SBR reader the type of the element directly in front (:2059): anything but that element itself and
                 * the reader switches the element's SBR off (aacsbr.c:996-1000) -- so it does for an LFE */
                if (prev_slot < 0 && last_cce < 0) return HEAAC_PARSE_ERR_DATA;   /* "SBR was found before the first channel element" */
                HeaacAacElementInfo *to;
                if (last_cce >= 0) {
                    /* the coupling element's own SBR (it goes through ff_sbr_apply when it couples AFTER_IMDCT, :1924) */
                    if (!cce->elem) return HEAAC_PARSE_ERR_UNSUPPORTED;
                    to = &cce->elem[last_cce];
                } else {
                    to = &elem[prev_slot];
                }
                if (to->sbr_payload_bit >= 0) return HEAAC_PARSE_ERR_UNSUPPORTED;  /* a second payload for the element */
                to->sbr_payload_bit = at;
                to->sbr_payload_bytes = bytes;
                to->sbr_crc = (uint8_t)crc;
                to->sbr_misplaced = (uint8_t)(prev_type != TYPE_SCE && prev_type != TYPE_CPE && prev_type != TYPE_CCE);
            }
            break;
        }
        default:
            return HEAAC_PARSE_ERR_UNSUPPORTED;
        }
        if (slot >= 0) prev_slot = slot;
        if (type < TYPE_DSE && type != TYPE_CCE) last_cce = -1;
        prev_type = type;
        if (b->over) return HEAAC_PARSE_ERR_OVERREAD;
        if (pc_left(b) < 3) return REF_OVERREAD(&lw->loop);                         /* :2072-2075 */
    }
    if (!n_seen) return HEAAC_PARSE_ERR_DATA;
    /* every coupling element against every output element: apply_channel_coupling compares the target list with the
     * element's place in ac->che[type][] (:1903-1933 hands it `i`), which a program config element makes its tag */
    for (int k = 0; k < HEAAC_MAX_CCE; k++) {
        if (!cbase[k].present) continue;
        for (int e = 0; e < ne; e++) {
            HeaacCceFrame *o = &cce->cce[e * HEAAC_MAX_CCE + k];
            *o = cbase[k];
            o->behind_target = (uint8_t)(elem[e].present && cbase[k].outputs_before > elem[e].seq);
            if ((r = cce_resolve(&lists[k], layout->elem[e].type, layout->elem[e].id, o)) < 0) return r;
        }
    }
    for (int k = 0; k < HEAAC_MAX_CCE; k++) {
        if (!cbase[k].present) continue;
        pc_win_store(wc[k], &cce->ics[k], &st[0].cce_window_sequence[cbase[k].elem_id], &st[0].cce_use_kb_window[cbase[k].elem_id]);
    }
    for (int e = 0; e < ne; e++) {
        if (!elem[e].present) continue;
        for (int c = 0; c < layout->elem[e].channels; c++)
            pc_win_store(w[e][c], &ics[e * 2 + c], &st[e].window_sequence[c], &st[e].use_kb_window[c]);
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->channels = layout->channels;
        info->bits_consumed = b->pos;
        info->sbr_payload_bit = -1;
        info->n_cce = n_cce;
    }
    return HEAAC_PARSE_OK;
}



int heaac_aac_parse_frame_layout_ex(const HeaacAacConfig *cfg, HeaacAacLayout *layout, HeaacAacStream *st,
                                    const uint8_t *au, int size,
                                    float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                                    HeaacAacElementInfo *elem, const HeaacCceOut *cce, HeaacAacFrameInfo *info)
{
    if (!cfg || !layout || !st || !au || size <= 0 || !coeffs || !ics || !tools || !elem ||
        cfg->sampling_index < 0 || cfg->sampling_index > 12 ||
        layout->n_elements < 1 || layout->n_elements > HEAAC_MAX_ELEMENTS ||
        (cce && (!cce->cce || !cce->coeffs || !cce->ics || !cce->tools)))
        return HEAAC_PARSE_ERR_ARG;
    const HeaacParseTables *pt = heaac_parse_tables();
    if (!pt) return HEAAC_PARSE_ERR_ARG;
    LayoutWalk lw;
    memset(&lw, 0, sizeof(lw));
    lw.at_slot = -1;
    const int r = layout_walk(cfg, layout, st, au, size, coeffs, ics, tools, elem, cce, info, pt, &lw);
    if (r >= 0) return r;
    /* Refused.  As for a one-element stream (unit_refused): where the refusal is the reference's own and no coupling
     * element has been read, the elements completed before it keep what their decoders did -- window history moved,
     * noise drawn, predictors stepped: their records stand, `present` and `seq` say which and in which order -- and
     * the element the refusal stands in is rewritten into records that do as much as its decoder had done. */
    HeaacAacFrameInfo fi = { 0, 0, -1, 0, 0, 0, 0, 0, 0 };
    const PcHost *why = lw.at_slot >= 0 ? &lw.at : &lw.loop;
    if (why->as_reference && (!lw.b.over || why->ref_overread) && !lw.n_cce) {
        fi.refused = HEAAC_REFUSED_AS_REFERENCE;
        int work = 0;
        const int main_profile = cfg->object_type == HEAAC_AOT_AAC_MAIN;
        for (int e = 0; e < layout->n_elements; e++) {
            if (!elem[e].present) continue;
            for (int c = 0; c < layout->elem[e].channels; c++) {
                st[e].window_sequence[c] = (uint8_t)PC_WS0(lw.w[e][c]);
                st[e].use_kb_window[c] = (uint8_t)PC_KB0(lw.w[e][c]);
                work |= main_profile || noise_draws(&tools[e].ch[c], 128);
            }
        }
        if (lw.at_slot >= 0) {
            const int e = lw.at_slot;
            HeaacAacFrameInfo part;
            unit_refused(cfg, &st[e], &lw.b, lw.w[e], &lw.at, 0, 2, coeffs + (size_t)e * 2048, &tools[e], &part);
            if (part.refused & HEAAC_REFUSED_RUN_TOOLS) {
                elem[e].present = 1;                   /* (type, tag and seq were set when the element began) */
                work = 1;
            }
        }
        if (work) fi.refused |= HEAAC_REFUSED_RUN_TOOLS;
    }
    if (info) *info = fi;
    return r;
}

/* ------------------------------------------------------------------------------------------ */
/* batch over streams                                                                            */
/* ------------------------------------------------------------------------------------------ */
typedef struct {
    const HeaacAacConfig *cfg; HeaacAacStream *st; const uint8_t *const *au; const int *size;
    float *coeffs; HeaacIcs *ics; HeaacToolsFrame *tools; HeaacAacFrameInfo *info; int *status;
    size_t lo, hi; int failed;
} Job;

static void *job_run(void *p)
{
    Job *j = (Job *)p;
    for (size_t f = j->lo; f < j->hi; f++) {
        const int r = heaac_aac_parse_frame(j->cfg, &j->st[f], j->au[f], j->size[f], j->coeffs + f * 2048,
                                            j->ics + f * 2, j->tools + f, j->info ? j->info + f : NULL);
        if (j->status) j->status[f] = r;
        j->failed += r != HEAAC_PARSE_OK;
    }
    return NULL;
}

int heaac_aac_parse_batch(const HeaacAacConfig *cfg, HeaacAacStream *st,
                          const uint8_t *const *au, const int *size, size_t n,
                          float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                          HeaacAacFrameInfo *info, int *status, int threads)
{
    if (!cfg || !st || !au || !size || !coeffs || !ics || !tools) return HEAAC_PARSE_ERR_ARG;
    if (!n) return 0;
    if (!heaac_parse_tables()) return HEAAC_PARSE_ERR_ARG;
    if (threads <= 0) threads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (threads < 1) threads = 1;
    if ((size_t)threads > n) threads = (int)n;
    if (threads > 256) threads = 256;
    Job jobs[256];
    pthread_t tid[256];
    for (int t = 0; t < threads; t++) {
        Job j = { cfg, st, au, size, coeffs, ics, tools, info, status, n * t / threads, n * (t + 1) / threads, 0 };
        jobs[t] = j;
    }
    int started = 0;
    for (int t = 1; t < threads; t++) {
        if (pthread_create(&tid[t], NULL, job_run, &jobs[t]) != 0) break;
        started = t;
    }
    job_run(&jobs[0]);
    for (int t = started + 1; t < threads; t++) job_run(&jobs[t]);     /* threads that could not start: inline */
    int failed = jobs[0].failed;
    for (int t = 1; t < threads; t++) {
        if (t <= started) pthread_join(tid[t], NULL);
        failed += jobs[t].failed;
    }
    return failed;
}
