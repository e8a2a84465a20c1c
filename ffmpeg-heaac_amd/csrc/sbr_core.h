/* sbr_core.h -- the SBR / Parametric Stereo payload walk of heaac_sbr_parse_device (include/heaac_parse.h), written
 * once for the host and the device, in the manner of parse_core.h (whose bit reader it uses).
 *
 * A second, independent writing of what sbr_parse.c's heaac_sbr_parse_payload and heaac_sbr_no_payload do for a unit
 * whose payload carries no header, or one that changes nothing: the crc bits and the header flag, the header fields
 * (read and compared, never applied), SCE / CPE data (grid, dtdf, invf, envelopes, noise, harmonics, coupling), the
 * extended data with the Parametric Stereo reader in it, and the emit of the HeaacSbrFrame / HeaacPsFrame records.
 * The band counts come from the stream's current HeaacSbrHeader (n[0], n[1], n_q) in the array the HE decode calls
 * take; nothing is derived here and no libm function is called.  k_parse.hip instantiates the walk one lane per unit,
 * and for the host (heaac_debug_sbr_parse_core, include/heaac_debug.h), where it is tested and fuzzed.
 *
 * It never decides a refusal and never registers a header.  Wherever the host call would return anything but
 * HEAAC_PARSE_OK / HEAAC_PARSE_NO_SBR, and for every header that resets or touches the derived record (the first of
 * a stream included), the walk gives the unit up with an SC_WHY_* reason.  So it needs none of the host parser's
 * roll-backs: it works straight on the OUT row of the stream state, which the caller has filled with the IN row, and
 * the caller copies the row again when the unit is given up.  The records of such a unit are unspecified.
 *
 * The caller zeroes the unit's HeaacSbrFrame and HeaacPsFrame ahead of the walk (the host parser's memsets).
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
const HeaacSbrParseTables *heaac_sbr_parse_tables(void);   /* sbr_parse_tables.c */
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

/* one code word: the symbol, or -1 for a prefix that is no code of the book (tree_read of parse_bits.h) */
SC_FN int sc_tree(const HeaacSbrParseTables *t, int book, PcBits *b)
{
    const uint32_t w = pc_peek32(b);
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
SC_FN int sc_huff(const HeaacSbrParseTables *t, int book, PcBits *b, int *bad)
{
    const int s = sc_tree(t, book, b);
    if (s < 0) { *bad = 1; return 0; }
    return s - t->bias[book];
}

/* ---- the header: read and compared with what the stream holds.  Non-zero if it resets the band tables or touches
 * the derived record (read_header of sbr_parse.c: reset, tables_touched); otherwise all it changes is start ---- */
SC_FN int sc_header(HeaacSbrStream *s, PcBits *b)
{
    const unsigned amp_res = pc_bit1(b), start_freq = pc_bits(b, 4), stop_freq = pc_bits(b, 4), xover = pc_bits(b, 3);
    pc_bits(b, 2);
    const unsigned extra_1 = pc_bit1(b), extra_2 = pc_bit1(b);
    unsigned freq_scale = 2, alter_scale = 1, noise_bands = 2;
    if (extra_1) { freq_scale = pc_bits(b, 2); alter_scale = pc_bit1(b); noise_bands = pc_bits(b, 2); }
    unsigned limiter_bands = 2, limiter_gains = 2, interpol_freq = 1, smoothing_mode = 1;
    if (extra_2) {
        limiter_bands = pc_bits(b, 2); limiter_gains = pc_bits(b, 2);
        interpol_freq = pc_bit1(b); smoothing_mode = pc_bit1(b);
    }
    if (!s->have_spectrum || start_freq != s->bs_start_freq || stop_freq != s->bs_stop_freq || xover != s->bs_xover_band ||
        freq_scale != s->bs_freq_scale || alter_scale != s->bs_alter_scale || noise_bands != s->bs_noise_bands)
        return 1;
    if (limiter_bands != s->bs_limiter_bands || limiter_gains != s->bs_limiter_gains || interpol_freq != s->bs_interpol_freq ||
        smoothing_mode != s->bs_smoothing_mode || amp_res != s->bs_amp_res_header)
        return 1;
    s->start = 1;
    return 0;
}

/* ---- the time / frequency grid, straight into the channel's state (read_grid of sbr_parse.c) ---- */
SC_FN int sc_grid(const HeaacSbrStream *s, PcBits *b, HeaacSbrChanState *c)
{
    const int L_old = c->bs_num_env;
    if (L_old > 5) return 1;                           /* (no state the parsers leave) */
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
        /* the middle noise border; with a variable trailing end and pointer 0 the reference's unsigned arithmetic takes
         * t_env[L + 1], what an earlier frame left there (sbr_parse.c: grid_noise_border_index) */
        int idx;
        if (cls == 0) idx = L >> 1;
        else if (trail_var) idx = pointer == 0 ? L + 1 : L - (pointer > 2 ? pointer - 1 : 1);
        else idx = pointer == 0 ? 1 : pointer == 1 ? L - 1 : pointer - 1;
        c->t_q[1] = c->t_env[idx];
    }
    c->e_a[0] = (int8_t)-(c->e_a[1] != L_old);
    int l_a = -1;
    if (trail_var) l_a = pointer ? L + 1 - pointer : -1;
    else if (cls == 2) l_a = pointer > 1 ? pointer - 1 : -1;
    c->e_a[1] = (int8_t)l_a;
    return 0;
}

/* the second channel of a coupled pair takes the first one's grid (copy_grid of sbr_parse.c) */
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

/* The envelopes (noise = 0: read_envelope of sbr_parse.c) or the noise floors (noise = 1: read_noise) of one channel.
 * One loop for both, so that the code books are walked from a single place: a value continues along time from the row
 * before it (for an envelope of another resolution from the band that covers it) or along frequency from its lower
 * neighbour, whose first value is sent plain. */
SC_FN void sc_facs(const HeaacSbrParseTables *t, const HeaacSbrStream *s, const HeaacSbrHeader *h, PcBits *b,
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
            if (df || j) v = sc_huff(t, df ? t_huff : f_huff, b, bad);
            else v = (int)pc_bits(b, start_bits);
            cur[j] = base + delta * v;
        }
    }
    for (int j = 0; j < stride; j++) rows[j] = rows[count * stride + j];
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

/* sbr_single_channel_element / sbr_channel_pair_element (read_sce, read_cpe of sbr_parse.c), as loops over the
 * channels so that each reader stands in one place.  A pair that is not coupled sends both channels' envelopes ahead
 * of both noise floors; a coupled pair and a single channel send them channel by channel. */
SC_FN int sc_element(const HeaacSbrParseTables *t, HeaacSbrStream *s, const HeaacSbrHeader *h, PcBits *b, int channels)
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
        for (int i = 0; i < 5; i++) c->bs_invf_mode[1][i] = c->bs_invf_mode[0][i];
        if (ch && coupled)
            for (int i = 0; i < 5; i++) c->bs_invf_mode[0][i] = s->data[0].bs_invf_mode[0][i];
        else
            for (int i = 0; i < h->n_q; i++) c->bs_invf_mode[0][i] = (uint8_t)pc_bits(b, 2);
    }
    const int by_channel = coupled || channels == 1;
    for (int k = 0; k < 2 * channels; k++) {
        const int noise = by_channel ? k & 1 : k >> 1, ch = by_channel ? k >> 1 : k & 1;
        sc_facs(t, s, h, b, &s->data[ch], ch, noise, &bad);
    }
    for (int ch = 0; ch < channels; ch++) sc_harmonics(h, b, &s->data[ch]);
    for (int ch = 0; ch < channels; ch++)
        if (!sc_facs_in_range(h, &s->data[ch])) return 1;
    return bad;
}

/* ---- Parametric Stereo (read_ps of sbr_parse.c; every error gives the unit up, so there is one cursor) ---- */

/* One envelope of one kind of parameter: a direction bit, then `count` code words.  Along frequency a value continues
 * from its lower neighbour, along time from the same band of the previous envelope (for envelope 0 the last one of
 * the previous frame).  Phases (modulo = 8) wrap; the others must stay within lo .. hi. */
SC_FN int sc_ps_envelope(const HeaacSbrParseTables *t, PcBits *b, const HeaacPsState *ps, int8_t (*par)[34], int count,
                         int book_df, int modulo, int lo, int hi, int e)
{
    const int along_time = (int)pc_bit1(b);
    const int book = book_df + along_time;
    const int bias = t->bias[book];
    const int src = e > 0 ? e - 1 : ps->num_env_old > 0 ? ps->num_env_old - 1 : 0;
    int run = 0;
    for (int band = 0; band < count; band++) {
        const int sym = sc_tree(t, book, b);
        if (sym < 0) return 1;
        run = (along_time ? par[src][band] : run) + sym - bias;
        if (modulo) run &= modulo - 1;
        else if (run < lo || run > hi) return 1;
        par[e][band] = (int8_t)run;
    }
    return 0;
}

/* The bits the SBR reader steps over, or -1 where the host's reader reports an error (ps_status != 0). */
SC_FN int sc_ps(const HeaacSbrParseTables *t, PcBits *b, HeaacPsState *ps, int bits_left_in_ext)
{
    const int at = b->pos;
    if (ps->num_env > 5 || ps->nr_iid_par > 34 || ps->nr_icc_par > 34 || ps->nr_ipdopd_par > 34) return -1;   /* (no state the parsers leave) */
    const int has_modes = (int)pc_bit1(b);
    if (has_modes) {
        if ((ps->enable_iid = (uint8_t)pc_bit1(b))) {
            const int mode = (int)pc_bits(b, 3);
            if (mode > 5) return -1;
            ps->nr_iid_par = (uint8_t)(mode % 3 == 0 ? 10 : mode % 3 == 1 ? 20 : 34);
            ps->nr_ipdopd_par = (uint8_t)(mode % 3 == 0 ? 5 : mode % 3 == 1 ? 11 : 17);
            ps->iid_quant = mode >= 3;
        }
        if ((ps->enable_icc = (uint8_t)pc_bit1(b))) {
            const int mode = (int)pc_bits(b, 3);
            if (mode > 5) return -1;
            ps->icc_mode = (uint8_t)mode;
            ps->nr_icc_par = (uint8_t)(mode % 3 == 0 ? 10 : mode % 3 == 1 ? 20 : 34);
        }
        ps->enable_ext = (uint8_t)pc_bit1(b);
    }
    /* envelope count and borders */
    ps->frame_class = (uint8_t)pc_bit1(b);
    const int code = (int)pc_bits(b, 2);
    ps->num_env_old = ps->num_env;
    ps->num_env = (uint8_t)(ps->frame_class ? code + 1 : code == 3 ? 4 : code);
    ps->border_position[0] = -1;
    for (int e = 1; e <= ps->num_env; e++)
        ps->border_position[e] = (int8_t)(ps->frame_class ? (int)pc_bits(b, 5) : e * 32 / ps->num_env - 1);
    const int top = ps->iid_quant ? 15 : 7;
    for (int kind = 0; kind < 2; kind++) {             /* IID, then ICC; a kind that is off reads as zeros */
        int8_t (*par)[34] = kind ? ps->icc_par : ps->iid_par;
        if (kind ? ps->enable_icc : ps->enable_iid) {
            for (int e = 0; e < ps->num_env; e++)
                if (sc_ps_envelope(t, b, ps, par, kind ? ps->nr_icc_par : ps->nr_iid_par,
                                   kind ? SC_PS_ICC_DF : ps->iid_quant ? SC_PS_IID_DF1 : SC_PS_IID_DF0, 0, kind ? 0 : -top,
                                   kind ? 7 : top, e))
                    return -1;
        } else {
            for (int e = 0; e < 5; e++)
                for (int k = 0; k < 34; k++) par[e][k] = 0;
        }
    }
    if (ps->enable_ext) {
        /* a byte count (escaped at 15), then extensions while a byte remains; id 0 carries the phases */
        int left = (int)pc_bits(b, 4);
        if (left == 15) left += (int)pc_bits(b, 8);
        left *= 8;
        while (left > 7) {
            const int id = (int)pc_bits(b, 2);
            const int from = b->pos;
            if (id == 0) {
                if ((ps->enable_ipdopd = (uint8_t)pc_bit1(b)))
                    for (int q = 0; q < 2 * ps->num_env; q++)    /* IPD, OPD per envelope (the host's reader does not look at their results either) */
                        sc_ps_envelope(t, b, ps, q & 1 ? ps->opd_par : ps->ipd_par, ps->nr_ipdopd_par,
                                       q & 1 ? SC_PS_OPD_DF : SC_PS_IPD_DF, 8, 0, 0, q >> 1);
                pc_bit1(b);
            }
            left -= 2 + (b->pos - from);
        }
        if (left < 0) return -1;
        b->pos += left;
    }
    /* the last envelope must reach slot 31: if not, or with none sent, one more repeats the last parameters known */
    const int n = ps->num_env;
    if (!(n && ps->border_position[n] >= 31)) {
        const int from = n ? n - 1 : (int)ps->num_env_old - 1;
        if (from >= 0 && from != n)
            for (int k = 0; k < 34; k++) {
                if (ps->enable_iid) ps->iid_par[n][k] = ps->iid_par[from][k];
                if (ps->enable_icc) ps->icc_par[n][k] = ps->icc_par[from][k];
                if (ps->enable_ipdopd) { ps->ipd_par[n][k] = ps->ipd_par[from][k]; ps->opd_par[n][k] = ps->opd_par[from][k]; }
            }
        ps->num_env = (uint8_t)(n + 1);
        ps->border_position[n + 1] = 31;
    }
    ps->is34bands_old = ps->is34bands;
    if (ps->enable_iid || ps->enable_icc)
        ps->is34bands = (ps->enable_iid && ps->nr_iid_par == 34) || (ps->enable_icc && ps->nr_icc_par == 34);
    if (!ps->enable_ipdopd)
        for (int e = 0; e < 5; e++)
            for (int k = 0; k < 34; k++) { ps->ipd_par[e][k] = 0; ps->opd_par[e][k] = 0; }
    if (has_modes) ps->start = 1;
    /* what the host parser refuses although the reference goes on: borders that do not ascend, values outside this
     * frame's quantiser in an envelope borrowed from an earlier one */
    for (int e = 0; e < ps->num_env; e++)
        if (ps->border_position[e] >= ps->border_position[e + 1]) return -1;
    for (int e = 0; e < ps->num_env; e++) {
        for (int k = 0; ps->enable_iid && k < ps->nr_iid_par; k++)
            if (ps->iid_par[e][k] < -top || ps->iid_par[e][k] > top) return -1;
        for (int k = 0; ps->enable_icc && k < ps->nr_icc_par; k++)
            if (ps->icc_par[e][k] < 0 || ps->icc_par[e][k] > 7) return -1;
    }
    const int used = b->pos - at;
    return used <= bits_left_in_ext ? used : -1;
}

/* ---- the records, into rows the caller has zeroed (emit_ps, emit_sbr of sbr_parse.c) ---- */
SC_FN void sc_emit_ps(const HeaacPsState *s, HeaacPsFrame *p)
{
    p->border_position[0] = -1;
    p->border_position[1] = 31;
    p->num_env = 1;
    p->nr_iid_par = p->nr_icc_par = 20;
    p->nr_ipdopd_par = 11;
    p->is34bands = s->is34bands;
    p->is34bands_old = s->is34bands_old;
    if (!s->start) return;
    p->start = 1;
    p->num_env = s->num_env;
    p->num_env_old = s->num_env_old;
    p->enable_ipdopd = s->enable_ipdopd;
    p->iid_quant = s->iid_quant;
    p->icc_mode = s->icc_mode;
    p->nr_iid_par = s->nr_iid_par ? s->nr_iid_par : 20;
    p->nr_icc_par = s->nr_icc_par ? s->nr_icc_par : 20;
    p->nr_ipdopd_par = s->nr_ipdopd_par ? s->nr_ipdopd_par : 11;
    for (int e = 0; e < 6; e++) p->border_position[e] = s->border_position[e];
    for (int e = 0; e < 5; e++) {
        for (int k = 0; k < 34; k++) { p->iid_par[e][k] = s->iid_par[e][k]; p->icc_par[e][k] = s->icc_par[e][k]; }
        for (int k = 0; k < 17; k++) { p->ipd_par[e][k] = s->ipd_par[e][k]; p->opd_par[e][k] = s->opd_par[e][k]; }
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
        if (!start) continue;
        o->bs_num_env = c->bs_num_env;
        o->bs_num_noise = c->bs_num_noise;
        o->bs_amp_res = c->bs_amp_res;
        o->bs_add_harmonic_flag = c->bs_add_harmonic_flag;
        for (int i = 0; i < 8; i++) { o->bs_freq_res[i] = c->bs_freq_res[i]; o->t_env[i] = c->t_env[i]; }
        for (int i = 0; i < 3; i++) o->t_q[i] = c->t_q[i];
        o->e_a[0] = c->e_a[0];
        o->e_a[1] = c->e_a[1];
        for (int i = 0; i < 5; i++) { o->bs_invf_mode[0][i] = c->bs_invf_mode[0][i]; o->bs_invf_mode[1][i] = c->bs_invf_mode[1][i]; }
        for (int i = 0; i < 48; i++) o->bs_add_harmonic[i] = c->bs_add_harmonic[i];
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
        if (sc_element(t, st, h, b, channels)) return SC_WHY_REFUSED;
        if (pc_bit1(b)) {                             /* bs_extended_data */
            int left = (int)pc_bits(b, 4);
            if (left == 15) left += (int)pc_bits(b, 8);
            left <<= 3;
            while (left > 7) {
                left -= 2;
                const int id = (int)pc_bits(b, 2);
                if (id == 2 && allow_ps) {            /* EXTENSION_ID_PS */
                    const int used = sc_ps(t, b, &st->ps, left);
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
