/* parse_streams.h -- the per-stream chain of heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams
 * (include/heaac_parse.h): T consecutive access units of one stream through pc_walk (parse_core.h) and, for HE-AAC,
 * sc_walk (sbr_core.h), each from the state the one before left, up to the first unit that is given up.  Written once
 * for the host and the device: k_parse_streams.hip instantiates pss_stream one lane per stream (k_parse_streams) and, through
 * pss_host, as heaac_debug_aac_parse_core_streams / heaac_debug_heaac_parse_core_streams (include/heaac_debug.h), where
 * it is tested, fuzzed (tests/c/fuzz_parse_streams.c) and debugged.  The one-unit call heaac_aac_parse_device and its
 * host form heaac_debug_aac_parse_core are the AAC chain at T = 1, one stream per unit.  Nothing of the syntax stands here.
 *
 * Stop rule.  t0 = the first unit either walk gives up from the state units 0 .. t0 - 1 left (an empty unit is one), or
 * T.  Units below t0 are HEAAC_PARSE_OK with the records of the one-unit calls; from t0 on the status is
 * HEAAC_PARSE_DEFERRED, the hold byte 1 and the records unspecified.  Both states stand as after unit t0 - 1, so the
 * host parser resumes at unit t0 with nothing to parse again.
 *
 * AAC state.  pc_walk reads *st at entry and stores into it on OK only.  Where sc_walk gives the same unit up, the AAC
 * half has committed already: the chain keeps the six bytes pc_walk may store (two channels' window sequence and
 * shape, mapped_tag, oc) from before the unit and puts them back.
 *
 * SBR state.  sc_walk works in place on the OUT row, which the caller filled with the IN row once per stream.  When it
 * gives unit t0 up the row is partly written; the chain copies the IN row again and walks the SBR half of units
 * 0 .. t0 - 1 a second time -- their HeaacAacFrameInfo is in memory, they are known to be taken, and they store the
 * same bytes into the same records.  That happens at most once per stream and call, since the stream stops there: no
 * scratch row, no per-unit row copy.
 *
 * The caller zeroes the HeaacToolsFrame, HeaacSbrFrame and HeaacPsFrame records of all T units ahead of the chain.
 *
 * Termination: the one loop makes at most 2 T passes (T forward, fewer than T in the second SBR walk); everything
 * inside is pc_walk's and sc_walk's, bounded by the unit's bits or a constant.  No byte outside
 * [offset[i], offset[i + 1]) of a unit is read.
 */
#ifndef HEAAC_PARSE_STREAMS_H
#define HEAAC_PARSE_STREAMS_H

#include "parse_core.h"
#include "sbr_core.h"

/* The geometry of every device parser (k_parse.hip, k_parse_streams.hip, the checks of capi.hip): one lane per unit or
 * per stream, one wave per block */
#define PARSE_BLOCK    64
#define PARSE_GRID_MAX (0x7fffffffull * PARSE_BLOCK)   /* lanes of the largest grid */
#define PARSE_MAX_UNIT (1u << 27)                      /* bytes: the walks count bits in an int */

/* `why` of the host forms: 0 for a unit that was taken; for unit t0 the PC_WHY_* reason of the AAC half, or
 * PSS_WHY_SBR * the SC_WHY_* reason where the SBR half gave it up; PSS_WHY_STOPPED for the units behind t0, which were
 * not looked at */
#define PSS_WHY_SBR     256
#define PSS_WHY_STOPPED (1 << 20)

/* One stream.  he: 0 compiles the SBR half out (a constant at every call site).  st: the stream's AAC state; sst_in /
 * sst_out: its two SBR rows (he only; the OUT row holds the IN row); off: the stream's T + 1 offsets into au; the
 * record pointers are those of the stream's unit 0.  status [T]; taken, hold [T] and why [T] may be NULL. */
SC_FN void pss_stream(const HeaacAacConfig *cfg, const HeaacParseTables *t, const uint32_t *lut, const HeaacSbrParseTables *stab,
                      const int he, HeaacAacStream *st, const HeaacSbrStream *sst_in, HeaacSbrStream *sst_out, const uint8_t *au,
                      const uint32_t *off, uint32_t T, int coeff_channels, float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                      HeaacAacFrameInfo *info, const HeaacSbrHeader *hdr, uint32_t n_hdr, HeaacSbrFrame *sbr, HeaacPsFrame *ps,
                      int32_t *status, uint32_t *taken, uint8_t *hold, int32_t *why)
{
    uint32_t t0 = T, end = T, u = 0;
    int again = 0, reason = 0;
    while (u < end) {
        const uint32_t lo = off[u], hi = off[u + 1];
        int r = PC_WHY_REFUSED;
        if (hi > lo && hi - lo < PARSE_MAX_UNIT) {
            const uint8_t k0 = st->window_sequence[0], k1 = st->window_sequence[1], k2 = st->use_kb_window[0],
                          k3 = st->use_kb_window[1], k4 = st->mapped_tag, k5 = st->oc;
            r = again ? 0 : pc_walk(cfg, t, lut, st, au + lo, (int)(hi - lo), coeff_channels,
                                    coeffs + (size_t)u * (size_t)coeff_channels * 1024, ics + (size_t)u * (size_t)coeff_channels,
                                    tools + u, info + u);
            if (he && !r) {
                const int rs = sc_walk(cfg, stab, sst_out, au + lo, (int)(hi - lo), info + u, hdr, n_hdr, sbr + u, ps ? ps + u : NULL);
                if (rs) {
                    /* (never in the second walk: the same bytes from the same state) */
                    r = PSS_WHY_SBR * rs;
                    st->window_sequence[0] = k0; st->window_sequence[1] = k1; st->use_kb_window[0] = k2;
                    st->use_kb_window[1] = k3; st->mapped_tag = k4; st->oc = k5;
                    const uint32_t *src = (const uint32_t *)sst_in;
                    uint32_t *dst = (uint32_t *)sst_out;
                    for (unsigned k = 0; k < sizeof(HeaacSbrStream) / 4; k++) dst[k] = src[k];
                    if (!again) {
                        again = 1;
                        t0 = u;
                        reason = r;
                        end = u;
                        u = 0;
                        continue;
                    }
                }
            }
        }
        if (r) {                                      /* the stream stops here */
            if (again) {                              /* (unreachable; the units from here on are given up as well) */
                if (u < t0) t0 = u;
                break;
            }
            t0 = u;
            reason = r;
            break;
        }
        u++;
    }
    for (u = 0; u < T; u++) {
        status[u] = u < t0 ? HEAAC_PARSE_OK : HEAAC_PARSE_DEFERRED;
        if (hold) hold[u] = u >= t0;
        if (why) why[u] = u < t0 ? 0 : u == t0 ? reason : PSS_WHY_STOPPED;
    }
    if (taken) *taken = t0;
}

/* The whole call on host memory: records zeroed, state rows copied, then stream by stream.  The arguments have passed
 * the checks of the entry points. */
SC_FN void pss_host(const HeaacAacConfig *cfg, const HeaacParseTables *t, const HeaacSbrParseTables *stab, const int he,
                    HeaacAacStream *st, const HeaacSbrStream *sst_in, HeaacSbrStream *sst_out, const uint8_t *au,
                    const uint32_t *off, size_t S, uint32_t T, int coeff_channels, float *coeffs, HeaacIcs *ics,
                    HeaacToolsFrame *tools, HeaacAacFrameInfo *info, const HeaacSbrHeader *hdr, uint32_t n_hdr, HeaacSbrFrame *sbr,
                    HeaacPsFrame *ps, int32_t *status, uint32_t *taken, uint8_t *hold, int32_t *why)
{
    const size_t n = S * T;
    sc_zero(tools, n * sizeof(*tools));
    if (he) {
        sc_copy(sst_out, sst_in, S * sizeof(*sst_out));
        sc_zero(sbr, n * sizeof(*sbr));
        if (ps) sc_zero(ps, n * sizeof(*ps));
    }
    for (size_t s = 0; s < S; s++) {
        const size_t i = s * T;
        pss_stream(cfg, t, &t->lut[0][0], stab, he, st + s, he ? sst_in + s : NULL, he ? sst_out + s : NULL, au, off + i, T, coeff_channels,
                   coeffs + i * (size_t)coeff_channels * 1024, ics + i * (size_t)coeff_channels, tools + i, info + i, hdr, n_hdr,
                   he ? sbr + i : NULL, he && ps ? ps + i : NULL, status + i, taken ? taken + s : NULL, hold ? hold + i : NULL, why ? why + i : NULL);
    }
}

#ifdef __HIPCC__
/* k_parse_streams.hip: the fill / copy kernel at the head of every device-parser call, on stream s.  tools, sbr and ps
 * [0 .. their words) = 0, st_out [0 .. st_words) = st_in [..]; the arrays are 4-byte aligned, every count may be 0 (its
 * pointers are then not looked at).  Internal to the library. */
__attribute__((visibility("hidden"))) void heaac_launch_parse_prep(void *tools, unsigned long long tools_words, const void *st_in,
                                                                   void *st_out, unsigned long long st_words, void *sbr,
                                                                   unsigned long long sbr_words, void *ps,
                                                                   unsigned long long ps_words, hipStream_t s);
#endif

#endif /* HEAAC_PARSE_STREAMS_H */
