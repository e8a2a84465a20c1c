// pipeline_layout.hip -- include/heaac_pipeline.h, second half: n streams of ONE multi-element layout (3.0 ... 7.1, a
// program config layout) advance in lock step, access units in host memory in, interleaved int16 PCM in host memory
// out.  What codec_layout.hip does for one stream with batches of one -- aac_decode_frame's element loop
// (aacdec.c:1999-2076), spectral_to_sample per element (:1903-1933), float_to_int16_interleave over output_data[]
// (:2096-2097) -- done for all streams at once, by the same rules (layout_common.hip: an element's shape, whether a
// unit stands, how an element's SBR record is read, the order of the spectral tools): the parsed records are laid out
// ELEMENT-major ([element][stream]), so every element of the layout is one batched tools call and one batched decode
// call over the n streams, and one interleave launch writes [n][len][channels].
//   * one noise generator per stream, run through the elements in bitstream order: the streams of a pipeline must
//     share that order (encoders emit one order; the first good unit sets it).  A stream that deviates, leaves an
//     element out or fails to parse gets silence for the tick and keeps its decoder state (as heaac_pipeline does);
//   * SBR per element (explicit signalling: m4ac.sbr = 1), "pure upsampling" where an element has no payload;
//   * coupling channel elements that a program config element names (up to HEAAC_MAX_CCE): one more batched
//     individual channel stream per slot (LpCoupled), their places in the unit the same for all streams of a tick.
// A tick's parse has two phases on the pool: phase 0 parses every unit into the set's records, submit() then drops
// the units that deviate from the tick (element order, coupling places), and phase 1 moves the host state of the
// streams that stand (window histories, SBR readers, coupling elements seen): a dropped stream's host state stays
// where its parked device rows stay.
// Two buffer sets rotate: the host parses tick t + 1 while tick t is on the link and on the GPU.
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stdlib.h>
#include <string.h>
#include "heaac_pipeline.h"
#include "codec_layout.h"        // heaac_sbr_output_mode
#include "layout_common.h"

#define LP_DEPTH 2
#define LP_MAX_HDRS 4096

struct LpElem : HeaacLayElem {      // out: 2 for an SCE with Parametric Stereo
    int cfg, words;                 // cfg_he or cfg_lc, as the pipeline has SBR or not
    float *d_state;                 // [n][words]
    HeaacPredictorState *d_pred;    // [n][channels][672] (AAC-Main) or NULL
    float *d_f32;                   // [n][channels][len]: the element's planes of the tick in work
    HeaacSbrStream *sst;            // [n] host: the element's SBR reader state per stream
};

// The coupling channel elements of a layout (slots 0 .. K-1 of the layout's list): individual channel streams of
// their own, batched per slot like an output element
struct LpCoupled {
    int K, words;                                   // words: 512 (the overlap), behind SBR a mono element's whole state
    float *d_state[HEAAC_MAX_CCE];                  // [n][words]: state of a coupling channel that couples AFTER_IMDCT
    HeaacPredictorState *d_pred[HEAAC_MAX_CCE];     // [n][672] (AAC-Main)
    float *d_ret[HEAAC_MAX_CCE];                    // [n][len]: the coupling channel's own output
    float *d_state_tmp;                             // [n][words]
    float *d_plane;                                 // [n][len]: one channel of a two-channel element, gathered for the coupling op
    HeaacSbrStream *sst[HEAAC_MAX_CCE];             // [n] host: a coupling channel's own SBR reader (che->sbr)
    unsigned char *seen;                            // [n][K]: an earlier unit of the stream carried the element
};

struct LpSet {
    // coupling elements: per output element the records that land there, per slot the channel's own records
    HeaacCceFrame *h_cce[HEAAC_MAX_ELEMENTS], *d_cce[HEAAC_MAX_ELEMENTS];   // [n][K]
    float *h_ccoef[HEAAC_MAX_CCE], *d_ccoef[HEAAC_MAX_CCE];                 // [n][1024]
    HeaacIcs *h_cics[HEAAC_MAX_CCE], *d_cics[HEAAC_MAX_CCE];
    HeaacToolsFrame *h_ctools[HEAAC_MAX_CCE], *d_ctools[HEAAC_MAX_CCE];
    HeaacSbrFrame *h_csbr[HEAAC_MAX_CCE], *d_csbr[HEAAC_MAX_CCE];
    float *d_ccoef_fm;                              // [n][K][1024]: the spectra frame-major, as the tools' POST half reads them
    HeaacCoupling *h_gain, *d_gain;                 // [ne][K][HEAAC_MAX_CCE_LINKS][n * len / 1024]: AFTER_IMDCT gains, call by call
    HeaacLayCcePlace *cpos;                         // [n][K]: where each coupling element stands
    unsigned *h_list, *d_list;                      // [2][2 n] (stream, parking row) pairs of the failed streams; then K x [2 n]:
                                                    // per coupling slot the streams whose element couples AFTER_IMDCT
    // per element, [n] each; pinned host / device
    float *h_coeffs[HEAAC_MAX_ELEMENTS], *d_coeffs[HEAAC_MAX_ELEMENTS];
    HeaacIcs *h_ics[HEAAC_MAX_ELEMENTS], *d_ics[HEAAC_MAX_ELEMENTS];
    HeaacToolsFrame *h_tools[HEAAC_MAX_ELEMENTS], *d_tools[HEAAC_MAX_ELEMENTS];
    HeaacSbrFrame *h_sbr[HEAAC_MAX_ELEMENTS], *d_sbr[HEAAC_MAX_ELEMENTS];
    HeaacPsFrame *h_ps[HEAAC_MAX_ELEMENTS], *d_ps[HEAAC_MAX_ELEMENTS];     // single channel elements with Parametric Stereo only
    int16_t *h_pcm, *d_pcm;
    unsigned char *failed;          // [n]
    unsigned char *seq;             // [n][ne] bitstream position of each element
    hipEvent_t done;
};

// What submit() settles about a tick before anything goes to the device
struct LpTick {
    size_t n_failed;
    HeaacLayCcePlace cpat[HEAAC_MAX_CCE];   // where the coupling elements stand, the same for all streams of the tick
    int n_cce;                              // ... and how many there are
    unsigned n_all, n_full;                 // pairs of the two failed lists (heaac_failed_lists)
};

struct HeaacLayoutPipeline {
    HeaacMem *mem;                  // every block but the parking area
    HeaacAacConfig aac;
    int ne, he, downsampled, len, main_profile;
    int out_channels;               // the layout's channels, plus one per SCE with Parametric Stereo
    size_t n;
    HeaacDevice *dev;
    hipStream_t run;
    LpElem e[HEAAC_MAX_ELEMENTS];
    LpSet set[LP_DEPTH];
    int32_t *d_rng;
    HeaacSbrHeader *d_hdr; size_t hdr_uploaded;
    HeaacSbrHeaderTable *tab;
    HeaacAacStream *ast;            // [n][ne]
    HeaacAacLayout *lay;            // [n]: every stream's own tag map
    // A good unit's effect on the stream's host state waits until submit() has checked it against the tick (element
    // order, coupling places): the parse (phase 0) leaves the new window histories and where the SBR payloads stand
    // here, and phase 1 commits them and reads the payloads -- for the streams still standing only.
    HeaacAacStream *ast_new;        // [n][ne]
    HeaacAacElementInfo *te_all;    // [n][ne]
    HeaacAacElementInfo *ce_all;    // [n][K]
    HeaacSbrStream *sst_tmp;        // HE: [threads] scratch SBR reader states, one per slice (slice 0's also serves submit())
    int have_order; unsigned char order[HEAAC_MAX_ELEMENTS];     // order[seq] = element at that bitstream position
    LpCoupled *cpl;                 // layouts whose program config element names coupling elements (AAC-LC / Main)
    // parked state of the streams whose unit failed
    float *d_park; size_t park_rows;
    unsigned long submitted, collected;
    HeaacPool *pool; int threads;   // threads: the pool's, the slices of a phase
    const uint8_t *const *job_au; const int *job_size; int *job_status; LpSet *job_set;
};

static inline HeaacSbrStream *sst_at(HeaacSbrStream *base, size_t i) { return (HeaacSbrStream *)((char *)base + i * heaac_sbr_stream_bytes()); }

// neutral records of one stream: silence, no tools, no SBR payload (from a COPY of the SBR reader state, made in the
// caller's scratch `tmp`).  keep_tools: the tools records and spectra are already what a refused unit leaves for the
// spectral tools.
static void neutral(HeaacLayoutPipeline *p, LpSet *s, size_t i, HeaacSbrStream *tmp, bool keep_tools = false)
{
    if (p->cpl) {
        const int K = p->cpl->K;
        for (int e = 0; e < p->ne; e++) memset(s->h_cce[e] + i * K, 0, (size_t)K * sizeof(HeaacCceFrame));
        for (int k = 0; k < K; k++) {
            memset(s->h_ccoef[k] + i * 1024, 0, 4096);
            memset(&s->h_cics[k][i], 0, sizeof(HeaacIcs));
            memset(&s->h_ctools[k][i], 0, sizeof(HeaacToolsFrame));
            if (p->he) heaac_lay_read_sbr(sst_at(p->cpl->sst[k], i), tmp, NULL, 0, NULL, 0, NULL, 1, &s->h_csbr[k][i], NULL);
        }
        memset(s->cpos + i * K, 0, (size_t)K * sizeof(HeaacLayCcePlace));
    }
    for (int k = 0; k < p->ne; k++) {
        const int ch = p->e[k].channels;
        memset(s->h_ics[k] + i * ch, 0, ch * sizeof(HeaacIcs));
        if (!keep_tools) {
            memset(s->h_coeffs[k] + i * (size_t)ch * 1024, 0, (size_t)ch * 4096);
            memset(&s->h_tools[k][i], 0, sizeof(HeaacToolsFrame));
        }
        if (p->he)
            heaac_lay_read_sbr(sst_at(p->e[k].sst, i), tmp, NULL, 0, NULL, 0, NULL, ch, &s->h_sbr[k][i], s->h_ps[k] ? &s->h_ps[k][i] : NULL);
    }
}

static HeaacSbrStream *slice_tmp(HeaacLayoutPipeline *p, int w) { return p->sst_tmp ? sst_at(p->sst_tmp, (size_t)w) : NULL; }

// Phase 0 of a tick: parse every unit of the slice into the set's records.  A refused unit gets neutral records here;
// a good one leaves its window histories and payload places in ast_new / te_all / ce_all, and nothing of the stream's
// host state moves yet (submit() may still drop it, lp_commit_slice then moves what is left).
// (this and lp_commit_slice out of line under their names: tests/test_pipeline.py looks the per-stream loops up)
__attribute__((noinline)) static void lp_parse_slice(HeaacLayoutPipeline *p, int w)
{
    const size_t lo = p->n * (size_t)w / (size_t)p->threads, hi = p->n * (size_t)(w + 1) / (size_t)p->threads;
    LpSet *s = p->job_set;
    const int ne = p->ne;
    HeaacSbrStream *tmp = slice_tmp(p, w);
    float *tc = (float *)malloc((size_t)ne * 2048 * sizeof(float));
    HeaacIcs *ti = (HeaacIcs *)malloc((size_t)ne * 2 * sizeof(HeaacIcs));
    HeaacToolsFrame *tt = (HeaacToolsFrame *)malloc((size_t)ne * sizeof(HeaacToolsFrame));
    HeaacAacElementInfo te[HEAAC_MAX_ELEMENTS];
    HeaacAacStream st[HEAAC_MAX_ELEMENTS];
    // the parser's coupling output (rows of HEAAC_MAX_CCE slots per output element)
    const int K = p->cpl ? p->cpl->K : 0;
    HeaacCceOut co = { NULL, NULL, NULL, NULL, NULL };
    HeaacAacElementInfo ce[HEAAC_MAX_CCE];
    if (K) {
        co.cce = (HeaacCceFrame *)malloc((size_t)ne * HEAAC_MAX_CCE * sizeof(HeaacCceFrame));
        co.coeffs = (float *)malloc(HEAAC_MAX_CCE * 4096);
        co.ics = (HeaacIcs *)malloc(HEAAC_MAX_CCE * sizeof(HeaacIcs));
        co.tools = (HeaacToolsFrame *)malloc(HEAAC_MAX_CCE * sizeof(HeaacToolsFrame));
        co.elem = ce;
        if (!co.cce || !co.coeffs || !co.ics || !co.tools) { free(tc); tc = NULL; }
    }
    for (size_t i = lo; i < hi; i++) {
        int r = HEAAC_PARSE_ERR_ARG;
        HeaacAacFrameInfo fi;
        memset(&fi, 0, sizeof(fi));
        if (tc && ti && tt) {
            // the parser works on copies of the window histories until the whole unit has parsed
            for (int k = 0; k < ne; k++) st[k] = p->ast[i * ne + k];
            r = heaac_aac_parse_frame_layout_ex(&p->aac, &p->lay[i], st, p->job_au[i], p->job_size[i], tc, ti, tt, te, K ? &co : NULL, &fi);
            if (r == HEAAC_PARSE_OK && !heaac_lay_unit_stands(te, ne, co.cce, K ? p->cpl->seen + i * K : NULL, K))
                r = HEAAC_PARSE_ERR_DATA;
        }
        if (p->job_status) p->job_status[i] = r;
        s->failed[i] = (unsigned char)(r != HEAAC_PARSE_OK);
        if (r != HEAAC_PARSE_OK) {
            // Where the refusal is the reference's own, what its element decoders had done by then stays done
            // (heaac_parse.h, HEAAC_REFUSED_*): the window histories the parser has moved, and -- through the records it
            // left for the elements marked present -- the noise generator and the predictors (failed = 2: the tools
            // run on them, submit() parks the DSP state rows only).
            if (r < 0 && tc && (fi.refused & HEAAC_REFUSED_AS_REFERENCE))
                for (int k = 0; k < ne; k++) p->ast[i * ne + k] = st[k];
            if (r < 0 && tc && (fi.refused & HEAAC_REFUSED_RUN_TOOLS)) {
                // (never once a coupling element has been read: lp_park leaves the coupling channels' rows alone)
                for (int k = 0; k < K; k++) assert(!ce[k].present);
                s->failed[i] = 2;
                for (int k = 0; k < ne; k++) {
                    const int ch = p->e[k].channels;
                    s->seq[i * ne + k] = te[k].present ? te[k].seq : 0xff;
                    if (te[k].present) {
                        memcpy(s->h_coeffs[k] + i * (size_t)ch * 1024, tc + (size_t)k * 2048, (size_t)ch * 4096);
                        s->h_tools[k][i] = tt[k];
                    } else {
                        memset(s->h_coeffs[k] + i * (size_t)ch * 1024, 0, (size_t)ch * 4096);
                        memset(&s->h_tools[k][i], 0, sizeof(HeaacToolsFrame));
                    }
                }
            }
            neutral(p, s, i, tmp, s->failed[i] == 2);
            continue;
        }
        for (int k = 0; k < K; k++) {
            const HeaacCceFrame &c0 = co.cce[k];            // (the same element in every output slot's row)
            s->cpos[i * K + k] = { c0.present, c0.outputs_before, c0.seq };
            p->ce_all[i * K + k] = ce[k];
            for (int e = 0; e < ne; e++) s->h_cce[e][i * K + k] = co.cce[e * HEAAC_MAX_CCE + k];
            if (c0.present) {
                memcpy(s->h_ccoef[k] + i * 1024, co.coeffs + k * 1024, 4096);
                s->h_cics[k][i] = co.ics[k];
                s->h_ctools[k][i] = co.tools[k];
            } else {
                memset(s->h_ccoef[k] + i * 1024, 0, 4096);
                memset(&s->h_cics[k][i], 0, sizeof(HeaacIcs));
                memset(&s->h_ctools[k][i], 0, sizeof(HeaacToolsFrame));
            }
        }
        for (int e = 0; K && e < ne; e++) heaac_lay_ltp_rule(&p->aac, s->h_cce[e] + i * K, K);
        for (int k = 0; k < ne; k++) {
            const int ch = p->e[k].channels;
            p->ast_new[i * ne + k] = st[k];
            p->te_all[i * ne + k] = te[k];
            s->seq[i * ne + k] = te[k].seq;
            memcpy(s->h_coeffs[k] + i * (size_t)ch * 1024, tc + (size_t)k * 2048, (size_t)ch * 4096);
            memcpy(s->h_ics[k] + i * ch, ti + k * 2, ch * sizeof(HeaacIcs));
            s->h_tools[k][i] = tt[k];
        }
    }
    free(tc); free(ti); free(tt);
    free(co.cce); free(co.coeffs); free(co.ics); free(co.tools);
}

// Phase 1: the streams whose unit submit() kept -- their window histories, the coupling elements they have carried,
// and their SBR payloads, read into the set's records (the readers and the header table move on here).
__attribute__((noinline)) static void lp_commit_slice(HeaacLayoutPipeline *p, int w)
{
    const size_t lo = p->n * (size_t)w / (size_t)p->threads, hi = p->n * (size_t)(w + 1) / (size_t)p->threads;
    LpSet *s = p->job_set;
    const int ne = p->ne;
    const int K = p->cpl ? p->cpl->K : 0;
    HeaacSbrStream *tmp = slice_tmp(p, w);
    for (size_t i = lo; i < hi; i++) {
        if (s->failed[i]) continue;
        for (int k = 0; k < ne; k++) p->ast[i * ne + k] = p->ast_new[i * ne + k];
        for (int k = 0; k < K; k++) {
            const HeaacLayCcePlace &cp = s->cpos[i * K + k];
            if (cp.present) p->cpl->seen[i * K + k] = 1;
            if (!p->he) continue;
            // A coupling channel's own SBR (it goes through ff_sbr_apply when it couples AFTER_IMDCT, aacdec.c:1920-1927).
            // A payload behind an element that couples in the spectrum is read all the same; without one the
            // reader's state only moves where the channel is transformed (the pipeline needs a record for every slot).
            const bool after = cp.present && s->h_cce[0][i * K + k].coupling_point == HEAAC_CC_AFTER_IMDCT;
            heaac_lay_read_sbr(sst_at(p->cpl->sst[k], i), after ? NULL : tmp, p->tab, p->aac.sample_rate, p->job_au[i], p->job_size[i],
                               cp.present ? &p->ce_all[i * K + k] : NULL, 1, &s->h_csbr[k][i], NULL);
        }
        if (!p->he) continue;
        for (int k = 0; k < ne; k++)
            heaac_lay_read_sbr(sst_at(p->e[k].sst, i), NULL, p->tab, p->aac.sample_rate, p->job_au[i], p->job_size[i],
                               &p->te_all[i * ne + k], p->e[k].channels, &s->h_sbr[k][i], s->h_ps[k] ? &s->h_ps[k][i] : NULL);
    }
}

static void lp_slice(void *ctx, int w, int phase)
{
    if (phase) lp_commit_slice((HeaacLayoutPipeline *)ctx, w);
    else lp_parse_slice((HeaacLayoutPipeline *)ctx, w);
}

extern "C" void heaac_layout_pipeline_destroy(HeaacLayoutPipeline *p)
{
    if (!p) return;
    heaac_pool_destroy(p->pool);
    if (p->run) (void)hipStreamSynchronize(p->run);
    for (int q = 0; q < LP_DEPTH; q++)
        if (p->set[q].done) (void)hipEventDestroy(p->set[q].done);
    heaac_mem_release(&p->mem);
    if (p->d_park) (void)hipFree(p->d_park);
    if (p->run) (void)hipStreamDestroy(p->run);
    heaac_sbr_table_destroy(p->tab);
    heaac_device_destroy(p->dev);
    free(p);
}

// the coupling channels' persistent side, and their records in the two buffer sets
static bool lp_coupled_create(HeaacLayoutPipeline *p, int K)
{
    const size_t n = p->n;
    HeaacMem **m = &p->mem;
    LpCoupled *c = NULL;
    if (!heaac_host(m, &c, sizeof(*c))) return false;
    p->cpl = c;
    c->K = K;
    c->words = p->he ? HEAAC_STATE_WORDS_HEV1_MONO : 512;
    const size_t sb = n * (size_t)c->words * 4;
    bool ok = heaac_host(m, &c->seen, n * K) && heaac_dev(m, &c->d_state_tmp, sb) && heaac_dev(m, &c->d_plane, n * (size_t)p->len * 4);
    for (int k = 0; ok && k < K; k++) {
        if (p->he) {
            ok = heaac_host(m, &c->sst[k], n * heaac_sbr_stream_bytes());
            if (ok) heaac_sbr_stream_init(c->sst[k], n);
        }
        ok = ok && heaac_dev(m, &c->d_state[k], sb) && hipMemset(c->d_state[k], 0, sb) == hipSuccess &&
             heaac_dev(m, &c->d_ret[k], n * (size_t)p->len * 4) &&
             (!p->main_profile || (heaac_dev(m, &c->d_pred[k], n * HEAAC_MAX_PREDICTORS * sizeof(HeaacPredictorState)) &&
                                   heaac_reset_predictors(c->d_pred[k], n * HEAAC_MAX_PREDICTORS)));
    }
    for (int q = 0; q < LP_DEPTH && ok; q++) {
        LpSet *s = &p->set[q];
        for (int e = 0; e < p->ne && ok; e++) ok = heaac_pair(m, &s->h_cce[e], &s->d_cce[e], n * K * sizeof(HeaacCceFrame));
        for (int k = 0; k < K && ok; k++)
            ok = heaac_pair(m, &s->h_ccoef[k], &s->d_ccoef[k], n * 4096) && heaac_pair(m, &s->h_cics[k], &s->d_cics[k], n * sizeof(HeaacIcs)) &&
                 heaac_pair(m, &s->h_ctools[k], &s->d_ctools[k], n * sizeof(HeaacToolsFrame)) &&
                 (!p->he || heaac_pair(m, &s->h_csbr[k], &s->d_csbr[k], n * sizeof(HeaacSbrFrame)));
        const size_t ng = (size_t)p->ne * K * HEAAC_MAX_CCE_LINKS * n * (p->len / 1024);
        ok = ok && heaac_dev(m, &s->d_ccoef_fm, n * K * 4096) && heaac_pair(m, &s->h_gain, &s->d_gain, ng * sizeof(HeaacCoupling)) &&
             heaac_host(m, &s->cpos, n * K * sizeof(HeaacLayCcePlace));
    }
    return ok;
}

extern "C" int heaac_layout_pipeline_create(HeaacLayoutPipeline **out, const HeaacAacConfig *aac, const HeaacAacLayout *layout,
                                            size_t n, int threads)
{
    if (!out) return HEAAC_ERR_ARG;
    *out = NULL;
    if (!aac || !layout || !n || layout->n_elements < 1 || layout->n_elements > HEAAC_MAX_ELEMENTS ||
        layout->channels < 1 || layout->channels > HEAAC_MAX_PCM_PLANES || aac->sampling_index < 0 || aac->sampling_index > 12 ||
        (aac->sbr != 0 && aac->sbr != 1))                 // implicit signalling (-1) is settled per stream by its first unit
        return HEAAC_ERR_ARG;
    // explicit SBR with Parametric Stereo on (or left open, which decode_audio_specific_config reads as on,
    // aacdec.c:476-477): every single channel element gives two channels
    HeaacLayShape sh;
    if (!heaac_lay_shape(layout, aac->sbr == 1, aac->ps != 0, &sh)) return HEAAC_ERR_ARG;
    HeaacLayoutPipeline *p = (HeaacLayoutPipeline *)calloc(1, sizeof(*p));
    if (!p) return HEAAC_ERR_NOMEM;
    HeaacMem **m = &p->mem;
    p->aac = *aac;
    p->ne = layout->n_elements;
    p->n = n;
    p->he = aac->sbr == 1;
    p->out_channels = sh.planes;
    const int mode = p->he ? heaac_sbr_output_mode(aac) : 0;
    if (mode < 0) { free(p); return HEAAC_ERR_ARG; }
    p->downsampled = mode;
    p->len = p->he && !mode ? 2048 : 1024;
    p->main_profile = aac->object_type == HEAAC_AOT_AAC_MAIN;
    int rc = heaac_device_create(&p->dev, n);
    if (rc != HEAAC_OK) { free(p); return rc; }
    bool ok = hipStreamCreateWithFlags(&p->run, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; ok && k < p->ne; k++) {
        LpElem &e = p->e[k];
        (HeaacLayElem &)e = sh.e[k];
        e.cfg = p->he ? e.cfg_he : e.cfg_lc;
        e.words = (int)heaac_cfg_shape(e.cfg).words;
        ok = heaac_dev(m, &e.d_state, n * (size_t)e.words * 4) && hipMemset(e.d_state, 0, n * (size_t)e.words * 4) == hipSuccess &&
             heaac_dev(m, &e.d_f32, n * (size_t)e.out * p->len * 4);
        if (ok && p->he) {
            ok = heaac_host(m, &e.sst, n * heaac_sbr_stream_bytes());
            if (ok) heaac_sbr_stream_init(e.sst, n);
        }
        if (ok && p->main_profile) {
            // every predictor of every channel
            const size_t np = n * (size_t)e.channels * HEAAC_MAX_PREDICTORS;
            ok = heaac_dev(m, &e.d_pred, np * sizeof(HeaacPredictorState)) && heaac_reset_predictors(e.d_pred, np);
        }
    }
    const int K = sh.cce_slots;
    if (ok && K) ok = lp_coupled_create(p, K);
    for (int q = 0; q < LP_DEPTH && ok; q++) {
        LpSet *s = &p->set[q];
        for (int k = 0; k < p->ne && ok; k++) {
            const size_t nc = n * (size_t)p->e[k].channels;
            ok = heaac_pair(m, &s->h_coeffs[k], &s->d_coeffs[k], nc * 4096) && heaac_pair(m, &s->h_ics[k], &s->d_ics[k], nc * sizeof(HeaacIcs)) &&
                 heaac_pair(m, &s->h_tools[k], &s->d_tools[k], n * sizeof(HeaacToolsFrame)) &&
                 (!p->he || heaac_pair(m, &s->h_sbr[k], &s->d_sbr[k], n * sizeof(HeaacSbrFrame))) &&
                 (p->e[k].cfg != HEAAC_CFG_HEV2 || heaac_pair(m, &s->h_ps[k], &s->d_ps[k], n * sizeof(HeaacPsFrame)));
        }
        ok = ok && heaac_pair(m, &s->h_pcm, &s->d_pcm, n * (size_t)p->out_channels * p->len * 2) &&
             heaac_host(m, &s->failed, n) && heaac_host(m, &s->seq, n * p->ne) &&
             heaac_pair(m, &s->h_list, &s->d_list, (4 + 2 * (size_t)K) * n * sizeof(unsigned)) &&
             hipEventCreate(&s->done) == hipSuccess;
    }
    ok = ok && heaac_dev(m, &p->d_rng, n * 4) && heaac_dev(m, &p->d_hdr, LP_MAX_HDRS * sizeof(HeaacSbrHeader)) &&
         heaac_seed_generators(p->d_rng, n);
    p->tab = heaac_sbr_table_create(LP_MAX_HDRS);
    ok = ok && p->tab && heaac_host(m, &p->ast, n * p->ne * sizeof(HeaacAacStream)) && heaac_host(m, &p->lay, n * sizeof(HeaacAacLayout)) &&
         heaac_host(m, &p->ast_new, n * p->ne * sizeof(HeaacAacStream)) && heaac_host(m, &p->te_all, n * p->ne * sizeof(HeaacAacElementInfo)) &&
         heaac_host(m, &p->ce_all, n * (size_t)(K ? K : 1) * sizeof(HeaacAacElementInfo));
    if (ok) {
        for (size_t i = 0; i < n; i++) p->lay[i] = *layout;
        // the null header (table entry 0) is what frames before their element's first header point at
        ok = hipMemcpy(p->d_hdr, heaac_sbr_table_data(p->tab), sizeof(HeaacSbrHeader), hipMemcpyHostToDevice) == hipSuccess;
        p->hdr_uploaded = 1;
    }
    if (ok) {
        if (threads <= 0) threads = heaac_threads_online_max32();
        if (threads > 256) threads = 256;
        if ((size_t)threads > n) threads = (int)n;
        ok = (p->pool = heaac_pool_create(threads, lp_slice, p)) != NULL;
        if (ok) p->threads = heaac_pool_threads(p->pool);
        ok = ok && (!p->he || heaac_host(m, &p->sst_tmp, p->threads * heaac_sbr_stream_bytes()));
    }
    if (!ok) { heaac_layout_pipeline_destroy(p); return HEAAC_ERR_NOMEM; }
    *out = p;
    return HEAAC_OK;
}

// ---------------------------------------------------------------------------
// a tick, stage by stage (heaac_layout_pipeline_submit below is the list)
// ---------------------------------------------------------------------------
// (every stage that walks the streams out of line under its name: tests/test_pipeline.py looks the per-stream loops up)

// stream i is out for the tick: silence, and its state stays where it was
static void lp_drop(HeaacLayoutPipeline *p, LpSet *s, size_t i, int *status, LpTick *t)
{
    s->failed[i] = 1;
    t->n_failed++;
    if (status) status[i] = HEAAC_PARSE_ERR_UNSUPPORTED;
    neutral(p, s, i, slice_tmp(p, 0));              // (slice 0 is the submitting thread's, and the pool is idle)
}

// What the units parsed in phase 0 make of the tick.  The element order of the pipeline's streams: the first good unit
// sets it, a stream that deviates is dropped for the tick.  Where the coupling elements stand among them, tick by tick:
// the first good stream of the tick says, the others must agree (the coupling POINT may differ from stream to stream).
__attribute__((noinline)) static void lp_settle(HeaacLayoutPipeline *p, LpSet *s, int *status, LpTick *t)
{
    const size_t n = p->n;
    const int ne = p->ne;
    memset(t, 0, sizeof(*t));
    for (size_t i = 0; i < n; i++) {
        const unsigned char *seq = s->seq + i * ne;
        if (s->failed[i] == 2) {
            // the elements a refused unit got through must stand where the pipeline's order has them: the generator
            // runs through the elements in that order.  (Else the unit is a failed one like any other: its status stands.)
            bool same = p->have_order != 0;
            for (int k = 0; same && k < ne; k++) same = seq[k] == 0xff || (seq[k] < ne && p->order[seq[k]] == k);
            if (!same) { s->failed[i] = 1; neutral(p, s, i, slice_tmp(p, 0)); }
        }
        if (s->failed[i]) { t->n_failed++; continue; }
        if (!p->have_order) {
            for (int k = 0; k < ne; k++) p->order[seq[k] < ne ? seq[k] : 0] = (unsigned char)k;
            p->have_order = 1;
        }
        bool same = true;
        for (int k = 0; k < ne; k++) same = same && seq[k] < ne && p->order[seq[k]] == k;
        if (!same) lp_drop(p, s, i, status, t);
    }
    const int K = p->cpl ? p->cpl->K : 0;
    int have_cpat = 0;
    for (size_t i = 0; K && i < n; i++) {
        if (s->failed[i]) continue;
        const HeaacLayCcePlace *cp = s->cpos + i * K;
        if (!have_cpat) { memcpy(t->cpat, cp, (size_t)K * sizeof(*cp)); have_cpat = 1; continue; }
        bool same = true;
        for (int k = 0; k < K; k++)
            same = same && cp[k].present == t->cpat[k].present &&
                   (!cp[k].present || (cp[k].outputs_before == t->cpat[k].outputs_before && cp[k].seq == t->cpat[k].seq));
        if (!same) lp_drop(p, s, i, status, t);
    }
    for (int k = 0; k < K; k++) t->n_cce += t->cpat[k].present;
}

// H2D (the run stream carries everything: the tick before has the GPU meanwhile)
static int lp_upload(HeaacLayoutPipeline *p, LpSet *s, const LpTick *t)
{
    const size_t n = p->n;
    const int K = p->cpl ? p->cpl->K : 0;
    const int rc = heaac_upload_headers(p->tab, &p->hdr_uploaded, p->d_hdr, NULL, p->run);
    if (rc != HEAAC_OK) return rc;
    for (int k = 0; k < p->ne; k++) {
        const size_t nc = n * (size_t)p->e[k].channels;
        HIP_OK(hipMemcpyAsync(s->d_coeffs[k], s->h_coeffs[k], nc * 4096, hipMemcpyHostToDevice, p->run));
        HIP_OK(hipMemcpyAsync(s->d_ics[k], s->h_ics[k], nc * sizeof(HeaacIcs), hipMemcpyHostToDevice, p->run));
        HIP_OK(hipMemcpyAsync(s->d_tools[k], s->h_tools[k], n * sizeof(HeaacToolsFrame), hipMemcpyHostToDevice, p->run));
        if (p->he) HIP_OK(hipMemcpyAsync(s->d_sbr[k], s->h_sbr[k], n * sizeof(HeaacSbrFrame), hipMemcpyHostToDevice, p->run));
        if (s->d_ps[k]) HIP_OK(hipMemcpyAsync(s->d_ps[k], s->h_ps[k], n * sizeof(HeaacPsFrame), hipMemcpyHostToDevice, p->run));
    }
    if (!t->n_cce) return HEAAC_OK;
    for (int e = 0; e < p->ne; e++)
        HIP_OK(hipMemcpyAsync(s->d_cce[e], s->h_cce[e], n * K * sizeof(HeaacCceFrame), hipMemcpyHostToDevice, p->run));
    for (int k = 0; k < K; k++) {
        HIP_OK(hipMemcpyAsync(s->d_ccoef[k], s->h_ccoef[k], n * 4096, hipMemcpyHostToDevice, p->run));
        HIP_OK(hipMemcpyAsync(s->d_cics[k], s->h_cics[k], n * sizeof(HeaacIcs), hipMemcpyHostToDevice, p->run));
        HIP_OK(hipMemcpyAsync(s->d_ctools[k], s->h_ctools[k], n * sizeof(HeaacToolsFrame), hipMemcpyHostToDevice, p->run));
        if (p->he) HIP_OK(hipMemcpyAsync(s->d_csbr[k], s->h_csbr[k], n * sizeof(HeaacSbrFrame), hipMemcpyHostToDevice, p->run));
    }
    return HEAAC_OK;
}

// rows of every failed stream: element states, predictors, noise generator -- to / from the parking area, which holds
// one region of `cap` rows per array.  n_all pairs at d_list: every failed stream; n_full at d_list + 2 n: those whose
// generator and predictors stay put as well (failed == 1; 2: the tools' side of the stream moves on).
// The coupling channels' state and predictor rows are not parked.  That is safe only because a failed stream carries
// all-zero coupling-element records (neutral() writes them, keep_tools or not), and for failed == 2 only because the
// parser never sets HEAAC_REFUSED_RUN_TOOLS once a coupling element has been read (asserted in lp_parse_slice).
static int lp_park(HeaacLayoutPipeline *p, LpSet *s, const LpTick *t, int restore)
{
    char *region = (char *)p->d_park;
    const size_t cap = p->park_rows;
    for (int k = 0; k < p->ne; k++) {
        const LpElem &e = p->e[k];
        const size_t sb = (size_t)e.words * 4, pb = (size_t)e.channels * HEAAC_MAX_PREDICTORS * sizeof(HeaacPredictorState);
        heaac_rows(p->run, s->d_list, t->n_all, 256, e.d_state, region, e.words, restore);
        region += cap * sb;
        if (e.d_pred) {
            if (t->n_full) heaac_rows(p->run, s->d_list + 2 * p->n, t->n_full, 256, e.d_pred, region, pb / 4, restore);
            region += cap * pb;
        }
    }
    if (t->n_full) heaac_rows(p->run, s->d_list + 2 * p->n, t->n_full, 64, p->d_rng, region, 1, restore);
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

// the failed streams' rows out of the way of the tick: the parking area grown to hold them, the lists, the rows
static int lp_park_failed(HeaacLayoutPipeline *p, LpSet *s, LpTick *t)
{
    if (!t->n_failed) return HEAAC_OK;
    size_t row = 4;
    for (int k = 0; k < p->ne; k++)
        row += (size_t)p->e[k].words * 4 + (p->e[k].d_pred ? (size_t)p->e[k].channels * HEAAC_MAX_PREDICTORS * sizeof(HeaacPredictorState) : 0);
    size_t rows;
    int rc = heaac_park_grow(p->run, t->n_failed, p->park_rows, 16, p->n, &rows);
    if (rc != HEAAC_OK) return rc;
    if (rows != p->park_rows) {
        if (p->d_park) (void)hipFree(p->d_park);
        p->d_park = NULL; p->park_rows = 0;
        if (!devmem((void **)&p->d_park, rows * row)) return HEAAC_ERR_NOMEM;
        p->park_rows = rows;
    }
    rc = heaac_failed_lists(p->run, s->failed, p->n, s->h_list, s->d_list, &t->n_all, &t->n_full);
    return rc == HEAAC_OK ? lp_park(p, s, t, 0) : rc;
}

// The spectral tools in the schedule's order (one noise generator per stream), every step one batched call over the n
// streams.  The second halves read the coupling channels' spectra frame-major, K slots per stream: gathered once
// every coupling element is through.
static int lp_run_tools(HeaacLayoutPipeline *p, LpSet *s, const LpTick *t)
{
    const size_t n = p->n;
    const int K = p->cpl ? p->cpl->K : 0;
    unsigned char pos[HEAAC_MAX_ELEMENTS];
    memset(pos, 0xff, sizeof(pos));
    for (int q = 0; q < p->ne; q++) pos[p->have_order ? p->order[q] : q] = (unsigned char)q;
    HeaacLayStep steps[HEAAC_LAY_MAX_STEPS];
    const int n_steps = heaac_lay_tools_schedule(t->cpat, K, pos, p->ne, steps);
    bool gathered = false;
    for (int i = 0; i < n_steps; i++) {
        const int k = steps[i].index;
        int rc;
        if (steps[i].cce) {
            rc = heaac_spectral_tools_batch_ex(p->dev, 1, HEAAC_TOOLS_ALL, s->d_ccoef[k], s->d_ctools[k], p->d_rng, p->d_rng,
                                               p->cpl->d_pred[k], p->cpl->d_pred[k], NULL, NULL, 0, n, (void *)p->run);
        } else if (steps[i].stages == HEAAC_TOOLS_POST) {
            for (int c = 0; c < K && !gathered; c++)
                HIP_OK(hipMemcpy2DAsync(s->d_ccoef_fm + (size_t)c * 1024, (size_t)K * 4096, s->d_ccoef[c], 4096, 4096, n,
                                        hipMemcpyDeviceToDevice, p->run));
            gathered = true;
            rc = heaac_spectral_tools_batch_ex(p->dev, p->e[k].channels, HEAAC_TOOLS_POST, s->d_coeffs[k], s->d_tools[k], NULL, NULL,
                                               NULL, NULL, s->d_cce[k], s->d_ccoef_fm, K, n, (void *)p->run);
        } else {
            rc = heaac_spectral_tools_batch_ex(p->dev, p->e[k].channels, steps[i].stages, s->d_coeffs[k], s->d_tools[k], p->d_rng, p->d_rng,
                                               p->e[k].d_pred, p->e[k].d_pred, NULL, NULL, 0, n, (void *)p->run);
        }
        if (rc != HEAAC_OK) return rc;
    }
    return HEAAC_OK;
}

// the streams whose coupling element of slot k couples AFTER_IMDCT this tick: their (stream, stream) pairs, and how many
__attribute__((noinline)) static unsigned lp_after_streams(const HeaacLayoutPipeline *p, const LpSet *s, int k, unsigned *lst)
{
    const int K = p->cpl->K;
    unsigned cnt = 0;
    for (size_t i = 0; i < p->n; i++) {
        if (s->failed[i] || !s->h_cce[0][i * K + k].present || s->h_cce[0][i * K + k].coupling_point != HEAAC_CC_AFTER_IMDCT) continue;
        lst[2 * cnt] = lst[2 * cnt + 1] = (unsigned)i;
        cnt++;
    }
    return cnt;
}

// The coupling channels that couple behind the IMDCT: their own IMDCT first (type 2 before types 1 and 0).  Only the
// streams whose element couples there this tick may move its overlap state: where all do the call works in place,
// where some do the others' rows are taken from a scratch copy of the state.
static int lp_coupling_channels(HeaacLayoutPipeline *p, LpSet *s, const LpTick *t)
{
    const size_t n = p->n;
    for (int k = 0; t->n_cce && k < p->cpl->K; k++) {
        if (!t->cpat[k].present) continue;
        unsigned *lst = s->h_list + (4 + 2 * (size_t)k) * n, *dl = s->d_list + (4 + 2 * (size_t)k) * n;
        const unsigned cnt = lp_after_streams(p, s, k, lst);
        if (!cnt) continue;
        float *st = p->cpl->d_state[k];
        const bool all = cnt == n;              // (no stream failed, then)
        const int rc = p->he
            ? heaac_he_decode_batch_ex(p->dev, HEAAC_CFG_HEV1_MONO, p->downsampled ? HEAAC_HE_DOWNSAMPLED : 0, s->d_ccoef[k], s->d_cics[k],
                                       s->d_csbr[k], p->d_hdr, LP_MAX_HDRS, NULL, st, all ? st : p->cpl->d_state_tmp, p->cpl->d_ret[k],
                                       HEAAC_PCM_F32_PLANAR, n, (void *)p->run)
            : heaac_lc_decode_batch(p->dev, 1, s->d_ccoef[k], s->d_cics[k], st, all ? st : p->cpl->d_state_tmp,
                                    p->cpl->d_ret[k], HEAAC_PCM_F32_PLANAR, n, (void *)p->run);
        if (rc != HEAAC_OK) return rc;
        if (all) continue;
        // rows of the streams that couple there, from the scratch copy (row i of it is stream i's)
        HIP_OK(hipMemcpyAsync(dl, lst, 2 * cnt * sizeof(unsigned), hipMemcpyHostToDevice, p->run));
        heaac_rows(p->run, dl, cnt, 256, st, p->cpl->d_state_tmp, (size_t)p->cpl->words, 1);
        HIP_OK(hipGetLastError());
    }
    return HEAAC_OK;
}

// one output element: its IMDCT, behind SBR everything else of ff_sbr_apply
static int lp_decode_element(HeaacLayoutPipeline *p, LpSet *s, int k)
{
    const LpElem &e = p->e[k];
    return p->he
        ? heaac_he_decode_batch_ex(p->dev, e.cfg, p->downsampled ? HEAAC_HE_DOWNSAMPLED : 0, s->d_coeffs[k], s->d_ics[k], s->d_sbr[k],
                                   p->d_hdr, LP_MAX_HDRS, s->d_ps[k], e.d_state, e.d_state, e.d_f32, HEAAC_PCM_F32_PLANAR, p->n, (void *)p->run)
        : heaac_lc_decode_batch(p->dev, e.channels, s->d_coeffs[k], s->d_ics[k], e.d_state, e.d_state, e.d_f32,
                                HEAAC_PCM_F32_PLANAR, p->n, (void *)p->run);
}

// Gain list l of coupling slot kc on element k, per stream (sub records each): the streams whose element couples
// AFTER_IMDCT and has that list -- with only >= 0 just those whose list lands on channel `only`.  The gain sits at the
// target channel (direct) or at channel 0 (gathered planes are one-channel frames).  used[c]: streams that target c.
__attribute__((noinline)) static void lp_gain_list(const HeaacLayoutPipeline *p, const LpSet *s, int k, int kc, int l, int only, bool direct,
                                                   HeaacCoupling *g, size_t used[2])
{
    const int K = p->cpl->K, sub = p->len / 1024;
    used[0] = used[1] = 0;
    for (size_t i = 0; i < p->n; i++) {
        const HeaacCceFrame &r = s->h_cce[k][i * K + kc];
        memset(&g[i * sub], 0, sub * sizeof(g[0]));
        if (s->failed[i] || !r.present || r.coupling_point != HEAAC_CC_AFTER_IMDCT || l >= r.n_links) continue;
        const int tch = r.link[l].target_ch < p->e[k].channels ? r.link[l].target_ch : 0;
        if (only >= 0 && tch != only) continue;
        for (int q = 0; q < sub; q++) {
            g[i * sub + q].on[direct ? tch : 0] = 1;
            g[i * sub + q].gain[direct ? tch : 0] = r.link[l].gain[0];
        }
        used[tch]++;
    }
}

// Every AFTER_IMDCT element in tag order, every gain list that lands on element k (apply_channel_coupling :1870-1898;
// apply_independent_coupling :1849-1862): one batched call per list, gains per stream.
// The batched op adds a [frames][1024] coupling signal into [frames][channels][1024] targets.  Planes of 1024 samples
// are that as they stand; planes of 2048 (behind SBR) are two such frames per stream with the stream's gain twice --
// for an element of one plane directly, for one of two planes channel by channel on a gathered copy of the plane
// (apply_independent_coupling runs over 1024 << sbr samples, aacdec.c:1849-1862).
static int lp_couple_after_imdct(HeaacLayoutPipeline *p, LpSet *s, const LpTick *t, int k)
{
    const LpElem &e = p->e[k];
    const size_t n = p->n;
    const int K = p->cpl ? p->cpl->K : 0, sub = p->len / 1024;
    const bool direct = sub == 1 || e.out == 1;
    for (int kc = 0; kc < K && t->n_cce; kc++) {
        if (!t->cpat[kc].present) continue;
        for (int l = 0; l < HEAAC_MAX_CCE_LINKS; l++) {
            HeaacCoupling *g = s->h_gain + (((size_t)k * K + kc) * HEAAC_MAX_CCE_LINKS + l) * n * sub;
            HeaacCoupling *dg = s->d_gain + (g - s->h_gain);
            size_t used[2], mine[2];
            lp_gain_list(p, s, k, kc, l, -1, direct, g, used);
            if (!used[0] && !used[1]) continue;
            if (direct) {
                HIP_OK(hipMemcpyAsync(dg, g, n * sub * sizeof(HeaacCoupling), hipMemcpyHostToDevice, p->run));
                const int rc = heaac_couple_after_imdct_batch(p->dev, sub == 1 ? e.out : 1, e.d_f32, p->cpl->d_ret[kc], dg, NULL,
                                                              n * sub, (void *)p->run);
                if (rc != HEAAC_OK) return rc;
                continue;
            }
            // two planes of 2048: a gain list lands on ONE channel per stream, and which one may differ from stream to
            // stream -- one pass per channel, each with the gains of the streams that target it
            for (int tc = 0; tc < 2; tc++) {
                if (!used[tc]) continue;
                if (used[tc ^ 1]) {
                    // mixed targets: this pass takes only the streams whose list lands on tc
                    lp_gain_list(p, s, k, kc, l, tc, false, g, mine);
                    HIP_OK(hipStreamSynchronize(p->run));      // (the staging area is about to be rewritten for the other channel)
                }
                HIP_OK(hipMemcpyAsync(dg, g, n * sub * sizeof(HeaacCoupling), hipMemcpyHostToDevice, p->run));
                const size_t row = (size_t)p->len * 4;
                HIP_OK(hipMemcpy2DAsync(p->cpl->d_plane, row, e.d_f32 + (size_t)tc * p->len, 2 * row, row, n, hipMemcpyDeviceToDevice, p->run));
                const int rc = heaac_couple_after_imdct_batch(p->dev, 1, p->cpl->d_plane, p->cpl->d_ret[kc], dg, NULL, n * sub, (void *)p->run);
                if (rc != HEAAC_OK) return rc;
                HIP_OK(hipMemcpy2DAsync(e.d_f32 + (size_t)tc * p->len, 2 * row, p->cpl->d_plane, row, row, n, hipMemcpyDeviceToDevice, p->run));
                if (used[tc ^ 1]) HIP_OK(hipStreamSynchronize(p->run));
            }
        }
    }
    return HEAAC_OK;
}

// the elements' planes interleaved, the failed streams' rows back and their PCM silent, the tick on its way to the host
static int lp_finish(HeaacLayoutPipeline *p, LpSet *s, const LpTick *t)
{
    HeaacPlaneRef planes[HEAAC_MAX_PCM_PLANES];
    for (int k = 0; k < p->ne; k++)
        for (int c = 0; c < p->e[k].out; c++) {
            planes[p->e[k].first_out + c].d_base = p->e[k].d_f32 + (size_t)c * p->len;
            planes[p->e[k].first_out + c].frame_stride = (size_t)p->e[k].out * p->len;
        }
    int rc = heaac_pcm_interleave_batch(p->dev, p->out_channels, planes, p->len, HEAAC_PCM_S16_INTERLEAVED, s->d_pcm, p->n, (void *)p->run);
    if (rc != HEAAC_OK) return rc;
    const size_t pcm_row = (size_t)p->out_channels * p->len;
    if (t->n_failed) {
        rc = lp_park(p, s, t, 1);
        if (rc != HEAAC_OK) return rc;
        heaac_rows(p->run, s->d_list, t->n_all, 256, s->d_pcm, NULL, pcm_row / 2, 2);      // (len is a multiple of 1024: whole 32-bit words)
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipMemcpyAsync(s->h_pcm, s->d_pcm, p->n * pcm_row * 2, hipMemcpyDeviceToHost, p->run));
    HIP_OK(hipEventRecord(s->done, p->run));
    return HEAAC_OK;
}

extern "C" int heaac_layout_pipeline_submit(HeaacLayoutPipeline *p, const uint8_t *const *au, const int *size, int *status)
{
    if (!p || !au || !size) return HEAAC_ERR_ARG;
    if (p->submitted - p->collected >= LP_DEPTH) return HEAAC_ERR_ARG;
    LpSet *s = &p->set[p->submitted % LP_DEPTH];
    // (the set's buffers are free: its last tick has been collected, which waited for its `done`)
    p->job_au = au; p->job_size = size; p->job_status = status; p->job_set = s;
    LpTick t;
    heaac_pool_run(p->pool, 0);
    lp_settle(p, s, status, &t);
    // the units that stand: now they move their streams' host state (a dropped one leaves it as its device rows are
    // left, parked -- as if the unit had never arrived)
    heaac_pool_run(p->pool, 1);
    if (heaac_sbr_table_count(p->tab) > LP_MAX_HDRS) return HEAAC_ERR_ARG;
    int rc = lp_upload(p, s, &t);
    if (rc == HEAAC_OK) rc = lp_park_failed(p, s, &t);
    if (rc == HEAAC_OK) rc = lp_run_tools(p, s, &t);
    if (rc == HEAAC_OK) rc = lp_coupling_channels(p, s, &t);
    for (int k = 0; rc == HEAAC_OK && k < p->ne; k++) {
        rc = lp_decode_element(p, s, k);
        if (rc == HEAAC_OK) rc = lp_couple_after_imdct(p, s, &t, k);
    }
    if (rc == HEAAC_OK) rc = lp_finish(p, s, &t);
    if (rc != HEAAC_OK) return rc;
    p->submitted++;
    return HEAAC_OK;
}

extern "C" int heaac_layout_pipeline_channels(const HeaacLayoutPipeline *p) { return p ? p->out_channels : 0; }

extern "C" int heaac_layout_pipeline_collect(HeaacLayoutPipeline *p, const int16_t **pcm)
{
    if (!p || !pcm || p->collected == p->submitted) return HEAAC_ERR_ARG;
    LpSet *s = &p->set[p->collected % LP_DEPTH];
    HIP_OK(hipEventSynchronize(s->done));
    *pcm = s->h_pcm;
    p->collected++;
    return HEAAC_OK;
}
