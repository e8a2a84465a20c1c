/* sbr_core.h -- the SBR / Parametric Stereo payload syntax (include/heaac_parse.h), written once for the host and the
 * device, in the manner of parse_core.h (whose bit reader it uses).
 *
 * The one writing of the payload: the header fields, SCE / CPE data (grid, dtdf, invf, envelopes, noise, harmonics,
 * coupling), the Parametric Stereo reader, and the emit of the HeaacSbrFrame / HeaacPsFrame records.  The bit order and
 * every value follow the reference: read_sbr_header (aacsbr.c:207-262), read_sbr_grid (:609-745), copy_sbr_grid
 * (:747-766), read_sbr_dtdf / read_sbr_invf / read_sbr_envelope / read_sbr_noise (:768-898),
 * read_sbr_single_channel_element / read_sbr_channel_pair_element (:928-980), ff_ps_read_data with its parameter readers
 * (aacps.c:84-279); the form is this project's own.  What the values must be is stated a second time, independently, by
 * the Python bit writer (tests/sbr_bitwriter.py), against which tests/test_sbr_parse.py compares.
 * The band counts come from the stream's current HeaacSbrHeader (n[0], n[1], n_q); nothing is derived here and no libm
 * function is called.
 *
 * Two callers.  sbr_parse.c (heaac_sbr_parse_payload, heaac_sbr_no_payload) calls the sc_* readers and adds what
 * belongs to the host: applying and registering a header, the roll-back of a refused element, the private PS cursor,
 * the statuses.  It is observable after an error, so the readers are host-exact on every exit: sc_element stops at the
 * bit the error was found at, and sc_ps leaves *ps as documented there and says which error it was.  sc_walk, below, is
 * the whole unit for the device (k_parse.hip, one lane per unit; heaac_debug_sbr_parse_core is its host form, tested
 * and fuzzed): it never decides a refusal and never registers a header.  Wherever the host call would return anything
 * but HEAAC_PARSE_OK / HEAAC_PARSE_NO_SBR, and for every header that resets or touches the derived record (the first of
 * a stream included), it gives the unit up with an SC_WHY_* reason.  So it needs none of the host's roll-backs: it
 * works straight on the OUT row of the stream state, which the caller has filled with the IN row, and the caller copies
 * the row again when the unit is given up.  The records of such a unit are unspecified.
 *
 * The caller zeroes the unit's HeaacSbrFrame and HeaacPsFrame ahead of sc_emit_* (a memset on the host, k_parse_prep on
 * the device).
 *
 * The code books are one flat table of tree nodes (HeaacSbrParseTables, 3.4 KB: on the device a copy in LDS), walked
 * bit by bit.  Per-band values are written into the state row and read back from there, so the walk keeps no
 * runtime-indexed private array.
 *
 * Termination: every loop is bounded by a constant -- 5 envelopes, 2 noise floors, 48 bands, 5 PS envelopes x 34
 * parameters, 32 bits of a code -- or by the extension's byte count (15 + 255), of which every pass takes two bits.
 */
#ifndef HEAAC_SBR_CORE_H
#define HEAAC_SBR_CORE_H

#include "parse_core.h"

#define HEAAC_ST_BOOKS 20             /* 0..9: the SBR books in the order of sbr_iso_tables.h, 10..19: the PS books */
#define HEAAC_ST_NODES 864            /* a complete book of n symbols has n - 1 inner nodes: 584 + 232, rounded up */

typedef struct HeaacSbrParseTables {
    int16_t  node[HEAAC_ST_NODES][2]; /* > 0: the child's index from the book's root, < 0: -(symbol + 1), 0: no code */
    uint16_t root[HEAAC_ST_BOOKS];    /* first node of each book */
    int8_t   bias[HEAAC_ST_BOOKS];    /* what a symbol carries above its value: sbr_huff_lav, ps_huff_offset */
    uint8_t  pad[4];
} HeaacSbrParseTables;                /* 3520 bytes, a multiple of 16 */

#ifdef __cplusplus
extern "C" {
#endif
const HeaacSbrParseTables *heaac_sbr_parse_tables(void);   /* sbr_parse.c; NULL: a book did not fit */
#ifdef __cplusplus
}
#endif

/* why a unit was given up (heaac_debug_sbr_parse_core reports it; the status of the call is HEAAC_PARSE_DEFERRED) */
#define SC_WHY_HEADER    1            /* a header that resets or touches the derived record: the host registers it */
#define SC_WHY_HDR_INDEX 2            /* the stream's header index lies outside d_hdr[n_hdr] */
#define SC_WHY_MISPLACED 4            /* a payload flagged sbr_misplaced */
#define SC_WHY_REFUSED   8            /* the host call would not return HEAAC_PARSE_OK for it */
#define SC_WHY_AAC       16           /* the unit's AAC status is not OK (set by the callers of the walk) */

enum { SC_T_ENV_15, SC_F_ENV_15, SC_T_ENV_BAL_15, SC_F_ENV_BAL_15, SC_T_ENV_30, SC_F_ENV_30, SC_T_ENV_BAL_30,
       SC_F_ENV_BAL_30, SC_T_NOISE_30, SC_T_NOISE_BAL_30,
       SC_PS_IID_DF1, SC_PS_IID_DT1, SC_PS_IID_DF0, SC_PS_IID_DT0, SC_PS_ICC_DF, SC_PS_ICC_DT, SC_PS_IPD_DF, SC_PS_IPD_DT,
       SC_PS_OPD_DF, SC_PS_OPD_DT };

/* On the device everything is inlined into the one kernel: a call would put the bit reader on the stack. */
#if defined(__HIPCC__)
#define SC_FN static __host__ __device__ __forceinline__
#else
#define SC_FN static inline
#endif

/* Rows are copied and cleared through the compiler's builtins, which it expands in line on the device and turns into
 * memcpy / memset on the host (byte loops cost the host parser a tenth of its time).  The functions of those names in
 * the HIP headers are not used: the compiler kept them as calls, and with them moved the code of the AAC walk kernel. */
#define sc_copy(dst, src, n) __builtin_memcpy(dst, src, n)
#define sc_zero(dst, n)      __builtin_memset(dst, 0, n)

/* One code word: the symbol, or -1 for a prefix that is no code of the book (the shipped books are complete: every
 * prefix is one).  The walk goes bit by bit through the flat table.  `lut`, where a caller has one (the host parser;
 * NULL on the device, whose 3.4 KB copy of the nodes in LDS is all it holds), is a table of the same codes by their first
 * SC_LUT_BITS bits, derived from the nodes (sbr_parse.c): lut[book][prefix] = length << 12 | symbol for a code no longer
 * than that, 0 for a longer one, which takes the walk.  It changes no result, only the time the codes take. */
#define SC_LUT_BITS 8
SC_FN int sc_tree(const HeaacSbrParseTables *t, const uint16_t *lut, int book, PcBits *b)
{
    const uint32_t w = pc_peek32(b);
    if (lut) {
        const unsigned e = lut[(book << SC_LUT_BITS) + (w >> (32 - SC_LUT_BITS))];
        if (e) { pc_skip(b, (int)(e >> 12)); return (int)(e & 0xfff); }
    }
    const int root = t->root[book];
    int at = root;
    for (int d = 0; d < 32; d++) {
        const int c = t->node[at][(w >> (31 - d)) & 1];
        if (c < 0) { pc_skip(b, d + 1); return -c - 1; }
        if (c == 0) return -1;
        at = root + c;
    }
    return -1;
}

/* a code word of an SBR book as the value it stands for; *bad is set for a prefix that is no code */
SC_FN int sc_huff(const HeaacSbrParseTables *t, const uint16_t *lut, int book, PcBits *b, int *bad)
{
    const int s = sc_tree(t, lut, book, b);
    if (s < 0) { *bad = 1; return 0; }
    return s - t->bias[book];
}

/* ---- the header (read_sbr_header, aacsbr.c:207-262): its fields as sent, defaults where a group is not.  The host
 * applies the record to the stream (sbr_parse.c), the device only compares it (sc_header) ---- */
typedef struct ScHeader {
    uint8_t amp_res, start_freq, stop_freq, xover_band, freq_scale, alter_scale, noise_bands;
    uint8_t limiter_bands, limiter_gains, interpol_freq, smoothing_mode;
} ScHeader;

SC_FN void sc_read_header(PcBits *b, ScHeader *hd)
{
    hd->amp_res = (uint8_t)pc_bit1(b);
    hd->start_freq = (uint8_t)pc_bits(b, 4);
    hd->stop_freq = (uint8_t)pc_bits(b, 4);
    hd->xover_band = (uint8_t)pc_bits(b, 3);
    pc_bits(b, 2);                                     /* bs_reserved */
    const unsigned extra_1 = pc_bit1(b), extra_2 = pc_bit1(b);
    hd->freq_scale = 2; hd->alter_scale = 1; hd->noise_bands = 2;
    if (extra_1) { hd->freq_scale = (uint8_t)pc_bits(b, 2); hd->alter_scale = (uint8_t)pc_bit1(b); hd->noise_bands = (uint8_t)pc_bits(b, 2); }
    hd->limiter_bands = 2; hd->limiter_gains = 2; hd->interpol_freq = 1; hd->smoothing_mode = 1;
    if (extra_2) {
        hd->limiter_bands = (uint8_t)pc_bits(b, 2); hd->limiter_gains = (uint8_t)pc_bits(b, 2);
        hd->interpol_freq = (uint8_t)pc_bit1(b); hd->smoothing_mode = (uint8_t)pc_bit1(b);
    }
}

/* the band tables must be rebuilt: no spectrum yet, or one of the six fields they are derived from changes */
SC_FN int sc_header_resets(const HeaacSbrStream *s, const ScHeader *hd)
{
    return !s->have_spectrum || hd->start_freq != s->bs_start_freq || hd->stop_freq != s->bs_stop_freq ||
           hd->xover_band != s->bs_xover_band || hd->freq_scale != s->bs_freq_scale ||
           hd->alter_scale != s->bs_alter_scale || hd->noise_bands != s->bs_noise_bands;
}

/* the limiter table (:258-259) and the four scalars live in the derived record: any change of them selects another
 * record without a reset */
SC_FN int sc_header_touches(const HeaacSbrStream *s, const ScHeader *hd)
{
    return hd->limiter_bands != s->bs_limiter_bands || hd->limiter_gains != s->bs_limiter_gains ||
           hd->interpol_freq != s->bs_interpol_freq || hd->smoothing_mode != s->bs_smoothing_mode ||
           hd->amp_res != s->bs_amp_res_header;
}

/* the device's use of a header: non-zero if the host must apply it; otherwise all it changes is start */
SC_FN int sc_header(HeaacSbrStream *s, PcBits *b)
{
    ScHeader hd;
    sc_read_header(b, &hd);
    if (sc_header_resets(s, &hd) || sc_header_touches(s, &hd)) return 1;
    s->start = 1;
    return 0;
}

/* ---- the time / frequency grid, straight into the channel's state.  VALUES as read_sbr_grid leaves them
 * (aacsbr.c:609-745).  sbr_grid() transmits, for each END of the frame that the frame class declares variable, an
 * absolute border and up to three relative borders walking inwards from it; a fixed end sits at slot 0 / 16 and has no
 * relative borders (FIXFIX instead spreads 1, 2 or 4 envelopes evenly).  Class bit 1 = the leading end is variable,
 * bit 0 = the trailing end is.  Non-zero for a grid that is refused: "too many SBR envelopes" in FIXFIX (> 4) or
 * VARVAR (> 5), found before the relative borders are read; two borders that meet or cross (the reference's uint8
 * arithmetic wraps a border walked below zero to > 235, which its own monotony check then refuses; meeting borders are
 * refused here as well, see heaac_parse.h) or a pointer beyond L + 1, found with the whole grid read.  The previous
 * frame's values move first, as in the reference, also when this grid is refused (the host rolls a refused element's
 * channel state back). ---- */
SC_FN int sc_grid(const HeaacSbrStream *s, PcBits *b, HeaacSbrChanState *c)
{
    /* L_old > 5: no state the parsers leave; with a corrupt caller-supplied row the guard keeps the host as well as
     * the device from indexing outside bs_freq_res[] and t_env[] */
    const int L_old = c->bs_num_env;
    if (L_old > 5) return 1;
    c->bs_freq_res[0] = c->bs_freq_res[L_old];
    c->t_env_num_env_old = c->t_env[L_old];
    const int cls = (int)pc_bits(b, 2);
    const int lead_var = (cls >> 1) & 1, trail_var = cls & 1;
    int L, pointer = 0;
    if (cls == 0) {                                    /* FIXFIX: 1, 2 or 4 envelopes spread evenly */
        L = 1 << pc_bits(b, 2);
        if (L > 4) return 1;
        const unsigned r = pc_bit1(b);
        c->t_env[0] = 0;
        for (int e = 1; e < L; e++) c->t_env[e] = (uint8_t)(e * (16 / L));
        c->t_env[L] = 16;
        for (int e = 0; e < L; e++) c->bs_freq_res[1 + e] = (uint8_t)r;
    } else {
        int lead_abs = 0, trail_abs = 16, n_lead = 0, n_trail = 0, crossed = 0;
        if (lead_var)  lead_abs = (int)pc_bits(b, 2);
        if (trail_var) trail_abs += (int)pc_bits(b, 2);
        if (lead_var)  n_lead = (int)pc_bits(b, 2);
        if (trail_var) n_trail = (int)pc_bits(b, 2);
        L = n_lead + n_trail + 1;
        if (L > 5) return 1;
        /* the relative borders walk inwards from either end; a border walked below zero is refused */
        int t = lead_abs;
        c->t_env[0] = (uint8_t)t;
        for (int i = 0; i < n_lead; i++) { t += 2 * (int)pc_bits(b, 2) + 2; c->t_env[1 + i] = (uint8_t)t; }
        t = trail_abs;
        c->t_env[L] = (uint8_t)t;
        for (int i = 0; i < n_trail; i++) {
            t -= 2 * (int)pc_bits(b, 2) + 2;
            crossed |= t < 0;
            c->t_env[L - 1 - i] = (uint8_t)t;
        }
        int nbits = 0;
        while ((1 << nbits) < L + 1) nbits++;          /* ceil(log2(L + 1)) <= 3 */
        pointer = (int)pc_bits(b, nbits);
        /* one resolution bit per envelope, last envelope first where only the trailing end is variable */
        for (int e = 0; e < L; e++) c->bs_freq_res[1 + (cls == 1 ? L - 1 - e : e)] = (uint8_t)pc_bit1(b);
        for (int e = 0; e < L; e++) crossed |= c->t_env[e] >= c->t_env[e + 1];
        if (crossed || pointer > L + 1) return 1;
    }
    c->bs_frame_class = (uint8_t)cls;
    c->bs_amp_res = (cls == 0 && L == 1) ? 0 : s->bs_amp_res_header;
    c->bs_num_env = (uint8_t)L;
    c->bs_num_noise = (uint8_t)(L > 1 ? 2 : 1);
    c->t_q[0] = c->t_env[0];
    c->t_q[c->bs_num_noise] = c->t_env[L];
    if (L > 1) {
        /* The middle noise border.  ISO/IEC 14496-3 4.6.18.3.3 counts the pointer from the variable end; the reference's
         * expression for a variable trailing end is `bs_num_env - FFMAX(bs_pointer - 1, 1)` on an UNSIGNED bs_pointer
         * (aacsbr.c:613, 729): with bs_pointer = 0 the subtraction wraps and the index comes out as L + 1, one past the
         * last border -- t_env[] keeps what an earlier frame with more envelopes left there (0 in a new stream).  The
         * reference is the contract, so the same entry is taken here (ISO would give L - 1); tests/test_sbr_parse.py
         * pins the case.  VARFIX counts from the leading end. */
        int idx;
        if (cls == 0) idx = L >> 1;
        else if (trail_var) idx = pointer == 0 ? L + 1 : L - (pointer > 2 ? pointer - 1 : 1);
        else idx = pointer == 0 ? 1 : pointer == 1 ? L - 1 : pointer - 1;
        c->t_q[1] = c->t_env[idx];
    }
    c->e_a[0] = (int8_t)-(c->e_a[1] != L_old);         /* l_APrev: the last frame's transient envelope was its last */
    int l_a = -1;                                      /* l_A: the envelope that starts at the transient, or -1 */
    if (trail_var) l_a = pointer ? L + 1 - pointer : -1;
    else if (cls == 2) l_a = pointer > 1 ? pointer - 1 : -1;
    c->e_a[1] = (int8_t)l_a;
    return 0;
}

/* the second channel of a coupled pair takes the first one's grid (copy_sbr_grid, aacsbr.c:747-766): its own carries
 * of the previous frame, then every transmitted grid field of the partner */
SC_FN int sc_copy_grid(HeaacSbrChanState *dst, const HeaacSbrChanState *src)
{
    const int L_old = dst->bs_num_env;
    if (L_old > 5) return 1;
    dst->bs_freq_res[0] = dst->bs_freq_res[L_old];
    dst->t_env_num_env_old = dst->t_env[L_old];
    dst->e_a[0] = (int8_t)-(dst->e_a[1] != L_old);
    dst->bs_frame_class = src->bs_frame_class;
    dst->bs_num_env = src->bs_num_env;
    dst->bs_num_noise = src->bs_num_noise;
    dst->bs_amp_res = src->bs_amp_res;
    dst->e_a[1] = src->e_a[1];
    for (int i = 0; i < 8; i++) dst->t_env[i] = src->t_env[i];
    for (int i = 1; i < 8; i++) dst->bs_freq_res[i] = src->bs_freq_res[i];
    for (int i = 0; i < 3; i++) dst->t_q[i] = src->t_q[i];
    return 0;
}

SC_FN void sc_dtdf(PcBits *b, HeaacSbrChanState *c)
{
    for (int i = 0; i < c->bs_num_env; i++)   c->bs_df_env[i]   = (uint8_t)pc_bit1(b);
    for (int i = 0; i < c->bs_num_noise; i++) c->bs_df_noise[i] = (uint8_t)pc_bit1(b);
}

/* The envelopes (noise = 0: read_sbr_envelope, aacsbr.c:783-858) or the noise floors (noise = 1: read_sbr_noise,
 * :860-898) of one channel.
 * One loop for both, so that the code books are walked from a single place: a value continues along time from the row
 * before it (for an envelope of another resolution from the band that covers it) or along frequency from its lower
 * neighbour, whose first value is sent plain. */
SC_FN void sc_facs(const HeaacSbrParseTables *t, const uint16_t *lut, const HeaacSbrStream *s, const HeaacSbrHeader *h, PcBits *b,
                   HeaacSbrChanState *c, int ch, int noise, int *bad)
{
    const int balance = s->bs_coupling && ch;
    const int delta = (ch == 1 && s->bs_coupling == 1) + 1;
    const int odd = h->n[1] & 1;
    const int start_bits = noise ? 5 : (balance ? 6 : 7) - (c->bs_amp_res != 0);
    const int t_huff = noise ? (balance ? SC_T_NOISE_BAL_30 : SC_T_NOISE_30)
                             : (c->bs_amp_res ? SC_T_ENV_30 : SC_T_ENV_15) + (balance ? 2 : 0);
    const int f_huff = noise ? (balance ? SC_F_ENV_BAL_30 : SC_F_ENV_30) : t_huff + 1;
    int32_t *rows = noise ? &c->noise_facs[0][0] : &c->env_facs[0][0];
    const int stride = noise ? 5 : 48, count = noise ? c->bs_num_noise : c->bs_num_env;
    for (int i = 0; i < count; i++) {
        const int res = !noise && c->bs_freq_res[i + 1] != 0, nb = noise ? h->n_q : h->n[res];
        const int same = noise || res == c->bs_freq_res[i];
        const int df = noise ? c->bs_df_noise[i] : c->bs_df_env[i];
        int32_t *cur = rows + (i + 1) * stride;
        const int32_t *prev = rows + i * stride;
        for (int j = 0; j < nb; j++) {
            int base = 0, v;
            if (df) base = prev[same ? j : res ? (j + odd) >> 1 : j ? 2 * j - odd : 0];
            else if (j) base = cur[j - 1];
            if (df || j) v = sc_huff(t, lut, df ? t_huff : f_huff, b, bad);
            else v = (int)pc_bits(b, start_bits);
            cur[j] = base + delta * v;
        }
    }
    sc_copy(rows, rows + count * stride, (size_t)stride * sizeof(*rows));
}

SC_FN void sc_harmonics(const HeaacSbrHeader *h, PcBits *b, HeaacSbrChanState *c)
{
    if ((c->bs_add_harmonic_flag = (uint8_t)pc_bit1(b)))
        for (int i = 0; i < h->n[1]; i++) c->bs_add_harmonic[i] = (uint8_t)pc_bit1(b);
}

/* the uint8 range of the frame record */
SC_FN int sc_facs_in_range(const HeaacSbrHeader *h, const HeaacSbrChanState *c)
{
    for (int e = 1; e <= c->bs_num_env; e++) {
        const int nb = h->n[c->bs_freq_res[e] != 0];
        for (int k = 0; k < nb; k++)
            if ((uint32_t)c->env_facs[e][k] > 255u) return 0;
    }
    for (int e = 1; e <= c->bs_num_noise; e++)
        for (int k = 0; k < h->n_q; k++)
            if ((uint32_t)c->noise_facs[e][k] > 255u) return 0;
    return 1;
}

/* sbr_single_channel_element / sbr_channel_pair_element (aacsbr.c:928-980), as loops over the channels so that each
 * reader stands in one place.  A pair that is not coupled sends both channels' envelopes ahead of both noise floors; a
 * coupled pair and a single channel send them channel by channel.  Non-zero for an element the host refuses
 * (HEAAC_PARSE_ERR_DATA): a grid error ends the read at once, a prefix that is no code (complete books: reachable
 * only past the end of the unit) or a value outside 0 .. 255 is reported with the whole element read. */
SC_FN int sc_element(const HeaacSbrParseTables *t, const uint16_t *lut, HeaacSbrStream *s, const HeaacSbrHeader *h, PcBits *b, int channels)
{
    int bad = 0;
    if (pc_bit1(b)) pc_bits(b, 4 * channels);          /* bs_data_extra: bs_reserved */
    if (channels == 2) s->bs_coupling = (uint8_t)pc_bit1(b);
    const int coupled = channels == 2 && s->bs_coupling;
    for (int ch = 0; ch < channels; ch++)
        if (ch && coupled ? sc_copy_grid(&s->data[1], &s->data[0]) : sc_grid(s, b, &s->data[ch])) return 1;
    for (int ch = 0; ch < channels; ch++) sc_dtdf(b, &s->data[ch]);
    for (int ch = 0; ch < channels; ch++) {
        HeaacSbrChanState *c = &s->data[ch];
        sc_copy(c->bs_invf_mode[1], c->bs_invf_mode[0], 5);
        if (ch && coupled)
            sc_copy(c->bs_invf_mode[0], s->data[0].bs_invf_mode[0], 5);
        else
            for (int i = 0; i < h->n_q; i++) c->bs_invf_mode[0][i] = (uint8_t)pc_bits(b, 2);
    }
    const int by_channel = coupled || channels == 1;
    for (int k = 0; k < 2 * channels; k++) {
        const int noise = by_channel ? k & 1 : k >> 1, ch = by_channel ? k >> 1 : k & 1;
        sc_facs(t, lut, s, h, b, &s->data[ch], ch, noise, &bad);
    }
    for (int ch = 0; ch < channels; ch++) sc_harmonics(h, b, &s->data[ch]);
    for (int ch = 0; ch < channels; ch++)
        if (!sc_facs_in_range(h, &s->data[ch])) return 1;
    return bad;
}

/* ---- Parametric Stereo.  VALUES as ff_ps_read_data leaves them (aacps.c:84-279); the form is this project's own:
 * ps_data() is read as a mode header, a time grid and then one block per parameter KIND (IID, ICC, and in the
 * extension IPD / OPD), each with its count, its two code books (along frequency, along time) and its range ---- */

/* One envelope of one kind of parameter: a direction bit, then `count` code words.  Along frequency a value continues
 * from its lower neighbour (from 0 for the first), along time from the same band of the previous envelope (for
 * envelope 0 the last one of the previous frame).  Phases (modulo = 8) wrap; the others must stay within lo .. hi.
 * Non-zero for a prefix that is no code (nothing more is stored) and for a value out of range (stored, as the
 * reference stores it, then refused). */
SC_FN int sc_ps_envelope(const HeaacSbrParseTables *t, const uint16_t *lut, PcBits *b, const HeaacPsState *ps, int8_t (*par)[34], int count,
                         int book_df, int modulo, int lo, int hi, int e)
{
    const int along_time = (int)pc_bit1(b);
    const int book = book_df + along_time;
    const int bias = t->bias[book];
    const int src = e > 0 ? e - 1 : ps->num_env_old > 0 ? ps->num_env_old - 1 : 0;
    int run = 0;
    for (int band = 0; band < count; band++) {
        const int sym = sc_tree(t, lut, book, b);
        if (sym < 0) return 1;
        run = (along_time ? par[src][band] : run) + sym - bias;
        if (modulo) run &= modulo - 1;
        par[e][band] = (int8_t)run;
        if (!modulo && (run < lo || run > hi)) return 1;
    }
    return 0;
}

#define SC_PS_ERR_DATA     (-1)       /* HEAAC_PARSE_ERR_DATA */
#define SC_PS_ERR_OVERREAD (-2)       /* HEAAC_PARSE_ERR_OVERREAD: a good frame that is longer than its extension */

/* ps_data() from the cursor b.  Returns the bits the SBR reader steps over, or SC_PS_ERR_* where the host reports an
 * error (ps_status != 0; the host then clears ps->start and skips the extension, sc_walk gives the unit up).  Later
 * frames read what an error leaves in *ps (num_env_old, the rows time deltas continue from, is34bands), so each exit
 * is part of the contract (tests/test_sbr_parse_error_state.py).  ERR_DATA:
 *   a reserved IID mode            the enable bit is stored, the counts are not
 *   a reserved ICC mode            enable_icc is stored, icc_mode is not (the reference stores the reserved value before
 *                                  refusing it)
 *   a prefix that is no code       nothing more is stored; the kinds behind it are not touched
 *   an IID / ICC value off range   the value is stored, the kinds behind it are not touched
 *   extensions past their count    refused at `left < 0`, with everything they carried stored
 *   a frame that is not usable     borders that do not ascend, or values outside the quantiser of THIS frame in an
 *                                  envelope borrowed from an earlier one (the reference goes on with both, see
 *                                  heaac_parse.h): the grid is closed, is34bands*, the zeroed phases and start = 1 are
 *                                  already written
 * ERR_OVERREAD: the same state as a good frame.  The cursor is wherever the read stopped: the host works on a private one. */
SC_FN int sc_ps(const HeaacSbrParseTables *t, const uint16_t *lut, PcBits *b, HeaacPsState *ps, int bits_left_in_ext)
{
    const int at = b->pos;
    /* no state the parsers leave; with a corrupt caller-supplied row the guard keeps the host as well as the device
     * from indexing outside the *_par rows and border_position[] */
    if (ps->num_env > 5 || ps->nr_iid_par > 34 || ps->nr_icc_par > 34 || ps->nr_ipdopd_par > 34) return SC_PS_ERR_DATA;
    const int has_modes = (int)pc_bit1(b);
    if (has_modes) {
        /* enable_ps_header: which kinds are on and at which resolution.  Mode 0..5 -> parameters per envelope (ISO/IEC
         * 14496-3 Table 8.4x): modes 3..5 repeat 0..2 with the fine IID quantiser */
        if ((ps->enable_iid = (uint8_t)pc_bit1(b))) {
            const int mode = (int)pc_bits(b, 3);
            if (mode > 5) return SC_PS_ERR_DATA;
            ps->nr_iid_par = (uint8_t)(mode % 3 == 0 ? 10 : mode % 3 == 1 ? 20 : 34);
            ps->nr_ipdopd_par = (uint8_t)(mode % 3 == 0 ? 5 : mode % 3 == 1 ? 11 : 17);
            ps->iid_quant = mode >= 3;
        }
        if ((ps->enable_icc = (uint8_t)pc_bit1(b))) {
            const int mode = (int)pc_bits(b, 3);
            if (mode > 5) return SC_PS_ERR_DATA;
            ps->icc_mode = (uint8_t)mode;
            ps->nr_icc_par = (uint8_t)(mode % 3 == 0 ? 10 : mode % 3 == 1 ? 20 : 34);
        }
        ps->enable_ext = (uint8_t)pc_bit1(b);
    }
    /* envelope count and borders: class 0 = 0, 1, 2 or 4 envelopes cutting the 32 slots evenly, class 1 = 1..4
     * envelopes with transmitted borders.  border_position[0] = -1. */
    ps->frame_class = (uint8_t)pc_bit1(b);
    const int code = (int)pc_bits(b, 2);
    ps->num_env_old = ps->num_env;
    ps->num_env = (uint8_t)(ps->frame_class ? code + 1 : code == 3 ? 4 : code);
    ps->border_position[0] = -1;
    for (int e = 1; e <= ps->num_env; e++)
        ps->border_position[e] = (int8_t)(ps->frame_class ? (int)pc_bits(b, 5) : e * 32 / ps->num_env - 1);
    const int top = ps->iid_quant ? 15 : 7;
    /* IID, then ICC.  A kind that is off reads as zeros (the reference clears its rows, aacps.c:204, 213): the records
     * carry the rows of every kind, and for all-zero values every count maps to the same thing (aacps.c:826-871) */
    for (int kind = 0; kind < 2; kind++) {
        int8_t (*par)[34] = kind ? ps->icc_par : ps->iid_par;
        if (kind ? ps->enable_icc : ps->enable_iid) {
            for (int e = 0; e < ps->num_env; e++)
                if (sc_ps_envelope(t, lut, b, ps, par, kind ? ps->nr_icc_par : ps->nr_iid_par,
                                   kind ? SC_PS_ICC_DF : ps->iid_quant ? SC_PS_IID_DF1 : SC_PS_IID_DF0, 0, kind ? 0 : -top,
                                   kind ? 7 : top, e))
                    return SC_PS_ERR_DATA;
        } else {
            sc_zero(par, 5 * 34);
        }
    }
    if (ps->enable_ext) {
        /* the extension container: a byte count (escaped at 15), then extensions while at least one byte remains; what
         * is left is padding.  Id 0 carries the phase parameters (IPD and OPD interleaved per envelope) and a reserved
         * bit; other ids carry nothing this decoder reads */
        int left = (int)pc_bits(b, 4);
        if (left == 15) left += (int)pc_bits(b, 8);
        left *= 8;
        while (left > 7) {
            const int id = (int)pc_bits(b, 2);
            const int from = b->pos;
            if (id == 0) {
                if ((ps->enable_ipdopd = (uint8_t)pc_bit1(b)))
                    for (int q = 0; q < 2 * ps->num_env; q++)    /* IPD, OPD per envelope; a bad prefix ends that envelope only */
                        sc_ps_envelope(t, lut, b, ps, q & 1 ? ps->opd_par : ps->ipd_par, ps->nr_ipdopd_par,
                                       q & 1 ? SC_PS_OPD_DF : SC_PS_IPD_DF, 8, 0, 0, q >> 1);
                pc_bit1(b);                                      /* reserved_ps */
            }
            left -= 2 + (b->pos - from);
        }
        if (left < 0) return SC_PS_ERR_DATA;
        b->pos += left;
    }
    /* The last envelope must reach the end of the frame (slot 31): if it does not -- or no envelope was sent -- one
     * more is appended that repeats the last parameters known (this frame's last envelope, or the previous frame's).
     * aacps.c:234-253. */
    const int n = ps->num_env;
    if (!(n && ps->border_position[n] >= 31)) {
        const int from = n ? n - 1 : (int)ps->num_env_old - 1;
        if (from >= 0 && from != n) {
            if (ps->enable_iid) sc_copy(ps->iid_par[n], ps->iid_par[from], 34);
            if (ps->enable_icc) sc_copy(ps->icc_par[n], ps->icc_par[from], 34);
            if (ps->enable_ipdopd) { sc_copy(ps->ipd_par[n], ps->ipd_par[from], 34); sc_copy(ps->opd_par[n], ps->opd_par[from], 34); }
        }
        ps->num_env = (uint8_t)(n + 1);
        ps->border_position[n + 1] = 31;
    }
    /* band layout of this frame: 34 bands as soon as one kind is sent at that resolution; a frame that sends neither
     * keeps the layout it had */
    ps->is34bands_old = ps->is34bands;
    if (ps->enable_iid || ps->enable_icc)
        ps->is34bands = (ps->enable_iid && ps->nr_iid_par == 34) || (ps->enable_icc && ps->nr_icc_par == 34);
    if (!ps->enable_ipdopd) {
        sc_zero(ps->ipd_par, sizeof(ps->ipd_par));
        sc_zero(ps->opd_par, sizeof(ps->opd_par));
    }
    if (has_modes) ps->start = 1;
    /* the frame that is not usable (see above) */
    for (int e = 0; e < ps->num_env; e++)
        if (ps->border_position[e] >= ps->border_position[e + 1]) return SC_PS_ERR_DATA;
    for (int e = 0; e < ps->num_env; e++) {
        for (int k = 0; ps->enable_iid && k < ps->nr_iid_par; k++)
            if (ps->iid_par[e][k] < -top || ps->iid_par[e][k] > top) return SC_PS_ERR_DATA;
        for (int k = 0; ps->enable_icc && k < ps->nr_icc_par; k++)
            if (ps->icc_par[e][k] < 0 || ps->icc_par[e][k] > 7) return SC_PS_ERR_DATA;
    }
    const int used = b->pos - at;
    return used <= bits_left_in_ext ? used : SC_PS_ERR_OVERREAD;
}

/* ---- the records, into rows the caller has zeroed ---- */
SC_FN void sc_emit_ps(const HeaacPsState *s, HeaacPsFrame *p)
{
    p->border_position[0] = -1;
    p->border_position[1] = 31;
    p->num_env = 1;
    p->nr_iid_par = p->nr_icc_par = 20;
    p->nr_ipdopd_par = 11;
    p->is34bands = s->is34bands;
    p->is34bands_old = s->is34bands_old;
    if (!s->start) return;                             /* mono copy: nothing else is read */
    p->start = 1;
    p->num_env = s->num_env;
    p->num_env_old = s->num_env_old;
    p->enable_ipdopd = s->enable_ipdopd;
    p->iid_quant = s->iid_quant;
    p->icc_mode = s->icc_mode;
    /* a parameter set that was never enabled has no count yet; its values are all zero, for which every count maps to
     * the same thing (aacps.c:826-871) */
    p->nr_iid_par = s->nr_iid_par ? s->nr_iid_par : 20;
    p->nr_icc_par = s->nr_icc_par ? s->nr_icc_par : 20;
    p->nr_ipdopd_par = s->nr_ipdopd_par ? s->nr_ipdopd_par : 11;
    sc_copy(p->border_position, s->border_position, 6);
    sc_copy(p->iid_par, s->iid_par, 5 * 34);
    sc_copy(p->icc_par, s->icc_par, 5 * 34);
    for (int e = 0; e < 5; e++) {
        sc_copy(p->ipd_par[e], s->ipd_par[e], 17);
        sc_copy(p->opd_par[e], s->opd_par[e], 17);
    }
}

SC_FN void sc_emit_sbr(const HeaacSbrStream *s, const HeaacSbrHeader *h, int channels, int start, int reset, HeaacSbrFrame *f)
{
    f->hdr = (uint16_t)s->hdr;
    f->start = (uint8_t)start;
    f->reset = (uint8_t)reset;
    f->kx_old = s->kx[0];
    f->m_old = s->m[0];
    f->bs_coupling = channels == 2 ? s->bs_coupling : 0;
    for (int ch = 0; ch < channels; ch++) {
        const HeaacSbrChanState *c = &s->data[ch];
        HeaacSbrChannel *o = &f->ch[ch];
        o->t_env_num_env_old = c->t_env_num_env_old;
        if (!start) continue;                          /* nothing else of the channel is read (h may be NULL) */
        o->bs_num_env = c->bs_num_env;
        o->bs_num_noise = c->bs_num_noise;
        o->bs_amp_res = c->bs_amp_res;
        o->bs_add_harmonic_flag = c->bs_add_harmonic_flag;
        sc_copy(o->bs_freq_res, c->bs_freq_res, 8);
        sc_copy(o->t_env, c->t_env, 8);
        sc_copy(o->t_q, c->t_q, 3);
        o->e_a[0] = c->e_a[0];
        o->e_a[1] = c->e_a[1];
        sc_copy(o->bs_invf_mode, c->bs_invf_mode, 10);
        sc_copy(o->bs_add_harmonic, c->bs_add_harmonic, 48);
        /* the bands of each envelope's resolution; what a state row holds beyond them is not data */
        for (int e = 0; e < c->bs_num_env; e++) {
            const int nb = h->n[c->bs_freq_res[e + 1] != 0];
            for (int k = 0; k < nb; k++) o->env_facs_q[e][k] = (uint8_t)c->env_facs[e + 1][k];
        }
        for (int e = 0; e < c->bs_num_noise; e++)
            for (int k = 0; k < h->n_q; k++) o->noise_facs_q[e][k] = (uint8_t)c->noise_facs[e + 1][k];
    }
}

/* One access unit.  *st: the OUT row of the stream's state, holding the IN row; info: what the AAC walk left for the
 * unit; hdr[n_hdr]: the derived headers; *sbr, *ps zeroed by the caller (ps may be NULL: no PS record, and no PS is
 * read).  Returns 0 -- *st, *sbr and *ps are what heaac_heaac_parse_frame_ex leaves behind its AAC half, returning
 * HEAAC_PARSE_OK or HEAAC_PARSE_NO_SBR -- or an SC_WHY_* reason (*st and the records unspecified: the caller copies
 * the IN row again). */
SC_FN int sc_walk(const HeaacAacConfig *cfg, const HeaacSbrParseTables *t, HeaacSbrStream *st, const uint8_t *au, int size,
                  const HeaacAacFrameInfo *info, const HeaacSbrHeader *hdr, uint32_t n_hdr, HeaacSbrFrame *sbr, HeaacPsFrame *ps)
{
    const int channels = info->channels, bit = info->sbr_payload_bit;
    if (channels != 1 && channels != 2) return SC_WHY_REFUSED;
    if (st->hdr >= n_hdr) return SC_WHY_HDR_INDEX;
    if (bit < 0 || cfg->sbr == 0) {                   /* heaac_sbr_no_payload */
        st->kx[0] = st->kx[1];
        st->m[0] = st->m[1];
        sc_emit_sbr(st, hdr, channels, 0, 0, sbr);
        if (ps) sc_emit_ps(&st->ps, ps);
        return 0;
    }
    if (info->sbr_misplaced) return SC_WHY_MISPLACED;
    if (bit > 8 * size || info->sbr_payload_bytes < 0) return SC_WHY_REFUSED;
    const int allow_ps = cfg->ps != 0 && channels == 1 && ps != NULL;
    PcBits bb, *b = &bb;
    pc_init(b, au, size);
    b->pos = bit;
    st->reset = 0;
    if (info->sbr_crc) pc_bits(b, 10);                /* bs_sbr_crc_bits: not checked by the reference either */
    st->kx[0] = st->kx[1];
    st->m[0] = st->m[1];
    if (pc_bit1(b) && sc_header(st, b)) return SC_WHY_HEADER;
    const HeaacSbrHeader *h = hdr + st->hdr;
    if (st->start) {
        if (h->n[0] > 24 || h->n[1] > 48 || h->n_q > 5) return SC_WHY_REFUSED;      /* (no header sbr_header.c builds) */
        if (sc_element(t, NULL, st, h, b, channels)) return SC_WHY_REFUSED;
        if (pc_bit1(b)) {                             /* bs_extended_data */
            int left = (int)pc_bits(b, 4);
            if (left == 15) left += (int)pc_bits(b, 8);
            left <<= 3;
            while (left > 7) {
                left -= 2;
                const int id = (int)pc_bits(b, 2);
                if (id == 2 && allow_ps) {            /* EXTENSION_ID_PS */
                    const int used = sc_ps(t, NULL, b, &st->ps, left);
                    if (used < 0) return SC_WHY_REFUSED;
                    left -= used;
                } else {                              /* PS signalled absent, or a reserved extension */
                    b->pos += left;
                    left = 0;
                }
            }
            if (left > 0) b->pos += left;
        }
    }
    if (b->over) return SC_WHY_REFUSED;
    sc_emit_sbr(st, h, channels, st->start, st->reset, sbr);
    if (ps) sc_emit_ps(&st->ps, ps);
    return 0;
}

#endif /* HEAAC_SBR_CORE_H */
