// layout_common.hip -- layout_common.h: the multi-element walk's rules, once for codec_layout.hip and pipeline_layout.hip.
#include <string.h>
#include "layout_common.h"

int heaac_lay_shape(const HeaacAacLayout *layout, int he, int ps_sce, HeaacLayShape *shape)
{
    memset(shape, 0, sizeof(*shape));
    for (int i = 0; i < layout->n_elements; i++) {
        HeaacLayElem &e = shape->e[i];
        e.channels = layout->elem[i].channels;
        e.cfg_lc = e.channels == 2 ? HEAAC_CFG_LC_STEREO : HEAAC_CFG_LC_MONO;
        e.cfg_he = e.channels == 2 ? HEAAC_CFG_HEV1 : HEAAC_CFG_HEV1_MONO;
        e.out = e.channels;
        if (he && ps_sce && layout->elem[i].type == HEAAC_ELEM_SCE) { e.cfg_he = HEAAC_CFG_HEV2; e.out = 2; }
        e.first_out = shape->planes;
        shape->planes += e.out;
    }
    for (int id = 0; id < 16; id++)
        if (layout->slot_of[HEAAC_ELEM_CCE][id] > shape->cce_slots) shape->cce_slots = layout->slot_of[HEAAC_ELEM_CCE][id];
    return shape->planes <= HEAAC_MAX_PCM_PLANES && shape->cce_slots <= HEAAC_MAX_CCE;
}

int heaac_lay_unit_stands(const HeaacAacElementInfo *elem, int ne, const HeaacCceFrame *cce, const unsigned char *seen, int K)
{
    for (int i = 0; i < ne; i++)
        if (!elem[i].present) return 0;
    for (int k = 0; k < K; k++)
        if (seen[k] && !cce[k].present) return 0;
    return 1;
}

void heaac_lay_ltp_rule(const HeaacAacConfig *cfg, HeaacCceFrame *row, int K)
{
    if (cfg->object_type != 4) return;
    for (int k = 0; k < K; k++)
        if (row[k].coupling_point != HEAAC_CC_AFTER_IMDCT) row[k].n_links = 0;
}

void heaac_lay_read_sbr(HeaacSbrStream *st, HeaacSbrStream *scratch, HeaacSbrHeaderTable *tab, int sample_rate,
                        const uint8_t *au, int size, const HeaacAacElementInfo *ei, int channels,
                        HeaacSbrFrame *sbr, HeaacPsFrame *ps)
{
    if (ei && ei->sbr_payload_bit >= 0) {
        (void)heaac_sbr_parse_payload(st, tab, sample_rate, au, size, ei->sbr_payload_bit, ei->sbr_payload_bytes, ei->sbr_crc, channels,
                                      (ei->sbr_misplaced ? HEAAC_SBR_MISPLACED : 0) | (ps ? HEAAC_SBR_ALLOW_PS : 0), sbr, ps, NULL);
        return;
    }
    if (scratch) {
        memcpy(scratch, st, heaac_sbr_stream_bytes());
        st = scratch;
    }
    heaac_sbr_no_payload(st, channels, sbr, ps);
}

int heaac_lay_tools_schedule(const HeaacLayCcePlace *cce, int K, const unsigned char *pos, int ne, HeaacLayStep *steps)
{
    int n_cce = 0, n = 0;
    for (int k = 0; k < K; k++) n_cce += cce[k].present != 0;
    for (int q = 0; q <= ne; q++) {
        for (int seq = 0; seq < n_cce; seq++)
            for (int k = 0; k < K; k++)
                if (cce[k].present && cce[k].outputs_before == q && cce[k].seq == seq)
                    steps[n++] = { 1, (unsigned char)k, HEAAC_TOOLS_ALL };
        for (int i = 0; q < ne && i < ne; i++)
            if (pos[i] == q) steps[n++] = { 0, (unsigned char)i, (unsigned char)(n_cce ? HEAAC_TOOLS_PRE : HEAAC_TOOLS_ALL) };
    }
    for (int i = 0; n_cce && i < ne; i++) steps[n++] = { 0, (unsigned char)i, HEAAC_TOOLS_POST };
    return n;
}
