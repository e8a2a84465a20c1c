// layout_common.h -- internal: the rules of the multi-element walk (aac_decode_frame's element loop and
// spectral_to_sample, aacdec.c:1903-1933, 1999-2076) that the layout codec context (codec_layout.hip, one stream,
// batches of one) and the layout pipeline (pipeline_layout.hip, n streams, element-major) share.  Each caller keeps
// its own buffers and batch size and executes what is decided here.  Not part of include/*.h.
#pragma once
#include "host_common.h"

// ---- element shapes ----
struct HeaacLayElem {
    int channels;                 // core channels
    int cfg_lc, cfg_he;           // HEAAC_CFG_* without / behind SBR
    int out, first_out;           // planes the element gives and where they stand among the stream's
};
struct HeaacLayShape {
    HeaacLayElem e[HEAAC_MAX_ELEMENTS];
    int planes;                   // of all elements
    int cce_slots;                // coupling channel elements the layout names: slots 0 .. cce_slots-1 of its list
};
// he: the stream has SBR.  ps_sce: with it, every single channel element carries Parametric Stereo and gives two
// planes (che_configure, aacdec.c:203-206; an LFE stays one channel, its type is not TYPE_SCE).
// 0: more than HEAAC_MAX_PCM_PLANES planes or HEAAC_MAX_CCE coupling slots.
int heaac_lay_shape(const HeaacAacLayout *layout, int he, int ps_sce, HeaacLayShape *shape);

// ---- does the unit stand ----
// Every element of the layout present, and every coupling element an earlier unit of the stream carried (seen[K]):
// the reference would transform, or couple, whatever the missing element's buffers still hold from an earlier frame,
// which no record of these paths carries.  cce: the K coupling records of output slot 0 (every row has the same elements).
int heaac_lay_unit_stands(const HeaacAacElementInfo *elem, int ne, const HeaacCceFrame *cce, const unsigned char *seen, int K);

// "Dependent coupling is not supported together with LTP" (apply_dependent_coupling :1822-1826 returns): an LTP
// profile stream (an ADTS header can say so) keeps its coupling elements but nothing couples in the spectrum.
// row: the K coupling records of one output slot.
void heaac_lay_ltp_rule(const HeaacAacConfig *cfg, HeaacCceFrame *row, int K);

// ---- an element's SBR record of one access unit ----
// ei with a payload: read it (a failed payload leaves its degraded record, start = 0, and the decode goes on, as
// ff_sbr_apply does; HEAAC_SBR_MISPLACED as the parser flagged it, HEAAC_SBR_ALLOW_PS where `ps` is given).
// ei NULL or without one: the "pure upsampling" record -- from st itself where scratch is NULL, else from a copy of
// st made in scratch (st does not move: the channel is not transformed this unit).
void heaac_lay_read_sbr(HeaacSbrStream *st, HeaacSbrStream *scratch, HeaacSbrHeaderTable *tab, int sample_rate,
                        const uint8_t *au, int size, const HeaacAacElementInfo *ei, int channels,
                        HeaacSbrFrame *sbr, HeaacPsFrame *ps);

// ---- the order of the spectral tools ----
// One noise generator runs through the elements in bitstream order.  A coupling element's tools as a whole at its
// place (nothing couples INTO it); an output element's as a whole at its place too, or, with coupling elements in the
// unit, its first half there and its second half -- coupling, TNS, coupling -- in layout order once every coupling
// element is through (spectral_to_sample walks the element types downwards, aacdec.c:1907).
struct HeaacLayStep { unsigned char cce, index, stages; };    // coupling slot (cce = 1) or output element `index`; HEAAC_TOOLS_*
#define HEAAC_LAY_MAX_STEPS (2 * HEAAC_MAX_ELEMENTS + HEAAC_MAX_CCE)
// a coupling element's place: behind `outputs_before` output elements, `seq`-th among the unit's coupling elements
struct HeaacLayCcePlace { unsigned char present, outputs_before, seq; };
// pos[ne]: the bitstream position of each output element (one whose position is not below ne gets no step: the
// elements a refused unit left out).  Returns the number of steps.
int heaac_lay_tools_schedule(const HeaacLayCcePlace *cce, int K, const unsigned char *pos, int ne, HeaacLayStep *steps);
