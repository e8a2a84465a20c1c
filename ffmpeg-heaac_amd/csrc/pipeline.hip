// pipeline.hip -- include/heaac_pipeline.h: access units in host memory -> int16 PCM in host memory, the four
// stages of consecutive ticks overlapped (host parse || H2D || GPU || D2H).
//
//   host parse   the worker pool of host_common.h, one slice of the streams per thread
//   H2D          stream `in`:  parsed records of the tick's buffer set, pinned -> device
//   GPU          stream `run`: heaac_spectral_tools_streams_ex + heaac_he_decode_streams_ex (AAC-LC:
//                heaac_lc_decode_streams_ex) over the T units of each stream, DSP state in place; a unit that did not
//                parse is held by the calls' masks.  A tick without one passes no mask, and with T = 1 the calls then
//                launch the batch kernels.
//   D2H          stream `out`: int16 PCM of the tick's buffer set, device -> pinned
// PL_DEPTH buffer sets rotate (set = tick % PL_DEPTH): a tick spends parse + H2D + GPU + D2H in flight (about 24 ms for
// 32 k streams) while the slowest stage takes 7 ms, so four ticks must overlap to keep every stage busy.
// Event order per set s:  in waits run_done[s] of the tick that used s last (its inputs are free again); run waits
// in_done[s] and that tick's out_done[s] (its PCM buffer is free); out waits run_done[s].
//
// HEAAC_PIPELINE_DEVICE_PARSE (heaac_pipeline_create_ex) replaces the first two stages: the tick's units are packed into
// one pinned byte buffer (pipeline_pack.h), uploaded, and parsed by the walk of k_parse_streams.hip on `in`, the parser
// states on the device; submit waits for the walk's stop positions and finishes the streams it stopped on the host pool
// from their gathered states, the records of those units scattered into the tick's rows (k_fix.hip) -- all on `in`, so
// the next tick's walk reads the states the fix-up left.  The GPU stage and the D2H are the same.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "heaac_pipeline.h"
#include "codec_layout.h"        // heaac_sbr_output_mode
#include "host_common.h"
#include "heaac_debug.h"
#include "pipeline_pack.h"

#define PL_MAX_HDRS 4096
#define PL_DEPTH HEAAC_PIPELINE_DEPTH

// The five record arrays of a tick or of the staging area, in the order of HeaacFixRows; sbr / ps are NULL where the
// configuration has none (HeaacPipeline::row_bytes says how long a unit's row is in each)
union Records {
    struct { float *coeffs; HeaacIcs *ics; HeaacToolsFrame *tools; HeaacSbrFrame *sbr; HeaacPsFrame *ps; };
    void *row[HEAAC_FIX_ARRAYS];
};
enum { REC_TOOLS = 2 };

struct Set {
    Records h, d;                   // pinned host (host parse only), device
    int16_t *h_pcm, *d_pcm;
    hipEvent_t in_start, in_done, run_done, out_done;
    int used;                       // a tick has gone through this set
    float parse_ms;
    // The hold masks of the streams calls, pinned (host parse only) / device.  [0, n T): hold_dsp, the unit's core
    // element did not parse; [n T, 2 n T): hold_tools, it did not and the spectral tools do not run either
    uint8_t *h_hold, *d_hold;
    int any_held;                   // some byte of hold_dsp is set (hold_tools is a subset): the masks are uploaded and passed
    // device parse: the tick's units laid end to end (grown on demand) and their offsets [nf + 1], pinned / device
    uint8_t *h_bytes, *d_bytes; size_t bytes_cap;
    uint32_t *h_off, *d_off;
};

// Device parse: the records the host parser made of the units the walk deferred, compact (staged unit u belongs at row
// dest[u] of the tick's arrays), pinned and device; grown on demand.  One area for all sets: `done` (recorded behind the
// scatter) says when the pinned half may be written again.
struct Staging {
    size_t cap;                     // units
    HeaacMem *mem;                  // every block of the area
    Records h, d;
    uint8_t *h_hold, *d_hold;       // [2 units]: hold_dsp of every staged unit, then hold_tools
    uint32_t *h_dest, *d_dest;
    hipEvent_t done; int used;
};

struct HeaacPipeline {
    HeaacMem *mem;                  // every block but the ones grown on demand (the sets' byte buffers, the staging area)
    HeaacAacConfig aac;
    int he_cfg, ncore, nout, he, out_len;
    size_t n, words;
    size_t row_bytes[HEAAC_FIX_ARRAYS];   // of one unit's row in each record array; 0: no such array
    size_t T, nf;                   // access units per stream and tick; n * T, the frames of a tick
    HeaacDevice *dev;
    hipStream_t in, run, out;
    Set set[PL_DEPTH];
    float *d_state; int32_t *d_rng;
    HeaacPredictorState *d_pred;  // AAC-Main streams: [n][ncore][672] (aacdec.c:1271-1322), else NULL
    int downsampled;              // SBR with the output at the core rate (aacsbr.c:1719)
    HeaacSbrHeader *d_hdr; size_t hdr_uploaded;
    HeaacSbrHeaderTable *tab;
    HeaacAacStream *ast; HeaacSbrStream *sst;
    unsigned long submitted, collected;
    float last_ms[4];
    HeaacPool *pool; int threads;   // threads: the pool's, the slices of a tick
    const uint8_t *const *job_au; const int *job_size; int *job_status; Set *job_set;
    unsigned long long n_device, n_host;    // heaac_pipeline_parse_counts
    // ---- HEAAC_PIPELINE_DEVICE_PARSE ----
    int dp;
    HeaacAacStream *d_ast;          // [n] parser states on the device (zeroed, as the host's calloc does)
    HeaacSbrStream *d_sst[2];       // HE: [n] each, ping-pong; d_sst[sst_cur] holds the streams' current rows
    int sst_cur;
    HeaacAacFrameInfo *d_info;      // [nf] what the AAC walk left per unit (the status kernel reads sbr_payload_bit)
    // What submit waits for is stored by the kernels into pinned host memory (m_*: the device's view of h_*): no
    // copy commands behind the kernels.
    int32_t *d_status, *h_status, *m_status;   // [nf] the walk's statuses; the host parser's, for the caller
    uint32_t *h_taken, *m_taken;    // [n] t0 of each stream
    hipEvent_t parsed;
    // the streams the walk stopped: their list and state rows, pinned / device ([n] rows: an HE stream's first header is
    // always deferred, so a first tick stops every stream)
    uint32_t *h_list, *d_list, *stop_base;
    HeaacAacStream *h_g_ast, *m_g_ast, *d_g_ast; HeaacSbrStream *h_g_sst, *m_g_sst, *d_g_sst;
    size_t m;                       // of the tick in submit
    Staging stg;
};

// One unit on its stream's parser states, its records into row f of r.  The core element did not parse (an SBR
// payload that fails leaves valid "SBR off" records and the unit decodes, as in the reference): the reference returns an
// error and writes no samples, aac_decode_frame :2065-2068; here *hold_dsp = 1 and the streams calls leave the stream's
// DSP state as it was and write silence, without reading the unit's records.  One thing does move, as in the
// reference: where its element decoders had drawn noise or stepped predictors before they refused the unit, the parser
// has left tools records that do exactly that much (HEAAC_REFUSED_RUN_TOOLS, heaac_parse.h) -- *hold_tools = 0 and the
// spectral tools run on them.  Returns the parser's status.  (The host-parse slices and the fix-up of a device-parse
// tick both come here.)
static inline int pl_parse_unit(HeaacPipeline *p, HeaacAacStream *ast, HeaacSbrStream *sst, const uint8_t *au, int size,
                                const Records *r, size_t f, uint8_t *hold_dsp, uint8_t *hold_tools)
{
    float *coeffs = r->coeffs + f * (size_t)p->ncore * 1024;
    HeaacIcs *ics = r->ics + f * p->ncore;
    HeaacAacFrameInfo fi;
    memset(&fi, 0, sizeof(fi));
    const int st = p->he
        ? heaac_heaac_parse_frame_ex(&p->aac, ast, sst, p->tab, au, size, p->ncore, coeffs, ics, &r->tools[f], &r->sbr[f],
                                     r->ps ? &r->ps[f] : NULL, &fi)
        : heaac_aac_parse_frame_ex(&p->aac, ast, au, size, p->ncore, coeffs, ics, &r->tools[f], NULL, &fi);
    const int core_failed = st < 0 && fi.channels == 0;
    const int run_tools = core_failed && (fi.refused & HEAAC_REFUSED_RUN_TOOLS);
    *hold_dsp = (uint8_t)core_failed;
    *hold_tools = (uint8_t)(core_failed && !run_tools);
    return st;
}

// The host-parse slice of a tick: each stream's T units in order on the stream's parser state, the records of unit t
// of stream i at i T + t.
// (out of line under this name, as fix_slice is: tests/test_pipeline.py looks the per-stream loops up in the library)
__attribute__((noinline)) static void parse_slice(HeaacPipeline *p, int w)
{
    const size_t lo = p->n * (size_t)w / (size_t)p->threads, hi = p->n * (size_t)(w + 1) / (size_t)p->threads;
    Set *s = p->job_set;
    for (size_t i = lo; i < hi; i++) {
        HeaacSbrStream *sst_i = (HeaacSbrStream *)((char *)p->sst + i * heaac_sbr_stream_bytes());
        for (size_t t = 0; t < p->T; t++) {
            const size_t f = i * p->T + t;
            const int r = pl_parse_unit(p, &p->ast[i], sst_i, p->job_au[f], p->job_size[f], &s->h, f, &s->h_hold[f],
                                        &s->h_hold[p->nf + f]);
            if (p->job_status) p->job_status[f] = r;
        }
    }
}

// Device parse, phase 1: the slice's units to their places in the set's byte buffer
static void pack_slice(HeaacPipeline *p, int w)
{
    const size_t lo = p->nf * (size_t)w / (size_t)p->threads, hi = p->nf * (size_t)(w + 1) / (size_t)p->threads;
    heaac_pack_bytes(p->job_au, p->job_size, p->job_set->h_off, lo, hi, p->job_set->h_bytes);
}

// Device parse, phase 2: the slice's share of the m stopped streams, each from its gathered states over its units
// t0 .. T - 1 into the staging rows stop_base says
__attribute__((noinline)) static void fix_slice(HeaacPipeline *p, int w)
{
    const size_t lo = p->m * (size_t)w / (size_t)p->threads, hi = p->m * (size_t)(w + 1) / (size_t)p->threads;
    Staging *g = &p->stg;
    const size_t units = p->stop_base[p->m];
    for (size_t j = lo; j < hi; j++) {
        const size_t i = p->h_list[j];
        HeaacSbrStream *sst_j = p->he ? (HeaacSbrStream *)((char *)p->h_g_sst + j * heaac_sbr_stream_bytes()) : NULL;
        for (size_t t = p->h_taken[i], u = p->stop_base[j]; t < p->T; t++, u++) {
            const size_t f = i * p->T + t;
            const int r = pl_parse_unit(p, &p->h_g_ast[j], sst_j, p->job_au[f], p->job_size[f], &g->h, u, &g->h_hold[u],
                                        &g->h_hold[units + u]);
            if (p->job_status) p->job_status[f] = r;
            g->h_dest[u] = (uint32_t)f;
        }
    }
}

static void pl_slice(void *ctx, int w, int phase)
{
    HeaacPipeline *p = (HeaacPipeline *)ctx;
    if (phase == 1) pack_slice(p, w);
    else if (phase == 2) fix_slice(p, w);
    else parse_slice(p, w);
}

// The configuration's record arrays for `units` units: device memory in *d, with pinned twins in *h unless NULL
static bool rec_alloc(const HeaacPipeline *p, HeaacMem **m, Records *h, Records *d, size_t units)
{
    for (int k = 0; k < HEAAC_FIX_ARRAYS; k++) {
        const size_t bytes = units * p->row_bytes[k];
        if (bytes && !(heaac_mem(m, HEAAC_MEM_DEVICE, &d->row[k], bytes) && (!h || heaac_mem(m, HEAAC_MEM_PINNED, &h->row[k], bytes))))
            return false;
    }
    return true;
}

// `units` rows of every record array, pinned -> device, on `in`
static int rec_upload(HeaacPipeline *p, const Records *h, const Records *d, size_t units, bool mono_tools)
{
    for (int k = 0; k < HEAAC_FIX_ARRAYS; k++) {
        if (!p->row_bytes[k]) continue;
        if (k == REC_TOOLS && mono_tools) {
            // a mono stream uses channel 0 of the tools record only: the second channel's 3.5 KB stay on the host
            // (the device copies were zeroed once and the kernel never reads them for one channel)
            HIP_OK(hipMemcpy2DAsync(d->tools, sizeof(HeaacToolsFrame), h->tools, sizeof(HeaacToolsFrame),
                                    offsetof(HeaacToolsFrame, ch) + sizeof(HeaacToolsChannel), units, hipMemcpyHostToDevice, p->in));
        } else {
            HIP_OK(hipMemcpyAsync(d->row[k], h->row[k], units * p->row_bytes[k], hipMemcpyHostToDevice, p->in));
        }
    }
    return HEAAC_OK;
}

static void stg_free(Staging *g)
{
    heaac_mem_release(&g->mem);
    g->cap = 0;
}

extern "C" void heaac_pipeline_destroy(HeaacPipeline *p)
{
    if (!p) return;
    heaac_pool_destroy(p->pool);
    if (p->in) (void)hipStreamSynchronize(p->in);
    if (p->run) (void)hipStreamSynchronize(p->run);
    if (p->out) (void)hipStreamSynchronize(p->out);
    for (int k = 0; k < PL_DEPTH; k++) {
        Set *s = &p->set[k];
        hipEvent_t ev[] = { s->in_start, s->in_done, s->run_done, s->out_done };
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (s->h_bytes) (void)hipHostFree(s->h_bytes);
        if (s->d_bytes) (void)hipFree(s->d_bytes);
    }
    stg_free(&p->stg);
    if (p->stg.done) (void)hipEventDestroy(p->stg.done);
    if (p->parsed) (void)hipEventDestroy(p->parsed);
    heaac_mem_release(&p->mem);
    if (p->in) (void)hipStreamDestroy(p->in);
    if (p->run) (void)hipStreamDestroy(p->run);
    if (p->out) (void)hipStreamDestroy(p->out);
    heaac_sbr_table_destroy(p->tab);
    heaac_device_destroy(p->dev);
    free(p);
}

extern "C" int heaac_pipeline_create(HeaacPipeline **out, const HeaacAacConfig *aac, int he_cfg, size_t n, int threads)
{
    return heaac_pipeline_create_streams(out, aac, he_cfg, n, 1, threads);
}

extern "C" size_t heaac_pipeline_frames_per_tick(const HeaacPipeline *p) { return p ? p->T : 0; }

extern "C" int heaac_pipeline_create_streams(HeaacPipeline **out, const HeaacAacConfig *aac, int he_cfg, size_t n_streams,
                                             size_t frames_per_tick, int threads)
{
    return heaac_pipeline_create_ex(out, aac, he_cfg, n_streams, frames_per_tick, threads, 0);
}

extern "C" void heaac_pipeline_parse_counts(const HeaacPipeline *p, unsigned long long counts[2])
{
    counts[0] = p ? p->n_device : 0;
    counts[1] = p ? p->n_host : 0;
}

extern "C" int heaac_pipeline_create_ex(HeaacPipeline **out, const HeaacAacConfig *aac, int he_cfg, size_t n_streams,
                                        size_t frames_per_tick, int threads, int flags)
{
    if (!out) return HEAAC_ERR_ARG;
    *out = NULL;
    const size_t n = n_streams, T = frames_per_tick;
    const bool lc = he_cfg == HEAAC_CFG_LC_MONO || he_cfg == HEAAC_CFG_LC_STEREO;
    if (!aac || !n || !T || n > SIZE_MAX / T ||
        (!lc && he_cfg != HEAAC_CFG_HEV2 && he_cfg != HEAAC_CFG_HEV1 && he_cfg != HEAAC_CFG_HEV1_MONO) ||
        aac->sampling_index < 0 || aac->sampling_index > 12)
        return HEAAC_ERR_ARG;
    if ((unsigned)flags & ~(unsigned)HEAAC_PIPELINE_DEVICE_PARSE) return HEAAC_ERR_ARG;
    const int dp = (flags & HEAAC_PIPELINE_DEVICE_PARSE) != 0;
    // what the device walk refuses (heaac_parse_args_ok of k_parse_streams.hip); its unit index is 32 bits wide
    if (dp && ((aac->object_type != HEAAC_AOT_AAC_LC && aac->object_type != HEAAC_AOT_AAC_MAIN) || n * T > 0xfffffffeull))
        return HEAAC_ERR_ARG;
    // (heaac_sbr_parse_args_ok: a mono configuration that signals Parametric Stereo takes PS records, which only
    // HEAAC_CFG_HEV2 has)
    if (dp && !lc && he_cfg != HEAAC_CFG_HEV2 && aac->ps != 0 && aac->chan_config == 1) return HEAAC_ERR_ARG;
    HeaacPipeline *p = (HeaacPipeline *)calloc(1, sizeof(*p));
    if (!p) return HEAAC_ERR_NOMEM;
    p->dp = dp;
    p->aac = *aac;
    p->he_cfg = he_cfg;
    p->he = !lc;
    // the configuration's two sample rates decide between 2048 samples at twice the core rate and "downsampled SBR"
    const int mode = lc ? 0 : heaac_sbr_output_mode(aac);
    if (mode < 0) { free(p); return HEAAC_ERR_ARG; }
    p->downsampled = mode;
    p->out_len = lc || mode ? 1024 : 2048;
    const HeaacCfgShape shape = heaac_cfg_shape(he_cfg);
    p->ncore = shape.ncore; p->nout = shape.nout; p->words = shape.words;
    p->n = n; p->T = T; p->nf = n * T;
    int rc = heaac_device_create(&p->dev, p->nf);
    if (rc != HEAAC_OK) { free(p); return rc; }
    // a T the HE streams call refuses on this device
    if (p->he && T > heaac_device_max_frames_per_stream(p->dev)) {
        heaac_device_destroy(p->dev);
        free(p);
        return HEAAC_ERR_ARG;
    }
    const size_t nf = p->nf;
    HeaacMem **m = &p->mem;
    bool ok = hipStreamCreateWithFlags(&p->in, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&p->run, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&p->out, hipStreamNonBlocking) == hipSuccess;
    const size_t row_bytes[HEAAC_FIX_ARRAYS] = { (size_t)p->ncore * 4096, p->ncore * sizeof(HeaacIcs), sizeof(HeaacToolsFrame),
                                                 p->he ? sizeof(HeaacSbrFrame) : 0,
                                                 he_cfg == HEAAC_CFG_HEV2 ? sizeof(HeaacPsFrame) : 0 };
    memcpy(p->row_bytes, row_bytes, sizeof(row_bytes));
    for (int k = 0; k < PL_DEPTH && ok; k++) {
        Set *s = &p->set[k];
        // (device parse: the records are made on the device, and what the host parser makes goes through the staging area)
        ok = rec_alloc(p, m, dp ? NULL : &s->h, &s->d, nf) &&
             (dp ? heaac_dev(m, &s->d_hold, 2 * nf) && heaac_pair(m, &s->h_off, &s->d_off, (nf + 1) * sizeof(uint32_t))
                 : heaac_pair(m, &s->h_hold, &s->d_hold, 2 * nf)) &&
             heaac_pair(m, &s->h_pcm, &s->d_pcm, nf * (size_t)p->nout * p->out_len * 2) &&
             hipEventCreate(&s->in_start) == hipSuccess && hipEventCreate(&s->in_done) == hipSuccess &&
             hipEventCreate(&s->run_done) == hipSuccess && hipEventCreate(&s->out_done) == hipSuccess;
        if (ok && !dp) {
            for (int a = 0; a < HEAAC_FIX_ARRAYS; a++) if (s->h.row[a]) memset(s->h.row[a], 0, nf * p->row_bytes[a]);
            ok = hipMemset(s->d.tools, 0, nf * sizeof(HeaacToolsFrame)) == hipSuccess;
        }
    }
    ok = ok && heaac_dev(m, &p->d_state, n * p->words * 4) && heaac_dev(m, &p->d_rng, n * 4) &&
         heaac_dev(m, &p->d_hdr, PL_MAX_HDRS * sizeof(HeaacSbrHeader)) &&
         hipMemset(p->d_state, 0, n * p->words * 4) == hipSuccess;
    if (ok && aac->object_type == HEAAC_AOT_AAC_MAIN) {
        // every predictor of every channel
        const size_t np = n * (size_t)p->ncore * HEAAC_MAX_PREDICTORS;
        ok = heaac_dev(m, &p->d_pred, np * sizeof(HeaacPredictorState)) && heaac_reset_predictors(p->d_pred, np);
    }
    ok = ok && heaac_seed_generators(p->d_rng, n);
    p->tab = heaac_sbr_table_create(PL_MAX_HDRS);
    ok = ok && p->tab &&
         (dp || (heaac_host(m, &p->ast, n * sizeof(HeaacAacStream)) && heaac_host(m, &p->sst, n * heaac_sbr_stream_bytes())));
    if (ok && dp) {
        ok = heaac_dev(m, &p->d_ast, n * sizeof(HeaacAacStream)) && heaac_dev(m, &p->d_info, nf * sizeof(HeaacAacFrameInfo)) &&
             heaac_pair(m, &p->h_status, &p->d_status, nf * sizeof(int32_t)) &&
             heaac_mem(m, HEAAC_MEM_PINNED, (void **)&p->h_taken, n * sizeof(uint32_t)) &&
             heaac_pair(m, &p->h_list, &p->d_list, n * sizeof(uint32_t)) && heaac_host(m, &p->stop_base, (n + 1) * sizeof(uint32_t)) &&
             heaac_pair(m, &p->h_g_ast, &p->d_g_ast, n * sizeof(HeaacAacStream)) &&
             (!p->he || (heaac_pair(m, &p->h_g_sst, &p->d_g_sst, n * sizeof(HeaacSbrStream)) &&
                         heaac_dev(m, &p->d_sst[0], n * sizeof(HeaacSbrStream)) && heaac_dev(m, &p->d_sst[1], n * sizeof(HeaacSbrStream)))) &&
             hipEventCreate(&p->parsed) == hipSuccess && hipEventCreate(&p->stg.done) == hipSuccess &&
             hipMemset(p->d_ast, 0, n * sizeof(HeaacAacStream)) == hipSuccess &&
             hipHostGetDevicePointer((void **)&p->m_status, p->h_status, 0) == hipSuccess &&
             hipHostGetDevicePointer((void **)&p->m_taken, p->h_taken, 0) == hipSuccess &&
             hipHostGetDevicePointer((void **)&p->m_g_ast, p->h_g_ast, 0) == hipSuccess &&
             (!p->he || hipHostGetDevicePointer((void **)&p->m_g_sst, p->h_g_sst, 0) == hipSuccess);
        if (ok && p->he) {
            // new streams, through the pinned rows the fix-up will use
            heaac_sbr_stream_init(p->h_g_sst, n);
            ok = hipMemcpy(p->d_sst[0], p->h_g_sst, n * sizeof(HeaacSbrStream), hipMemcpyHostToDevice) == hipSuccess;
        }
    }
    if (ok) {
        if (!dp) heaac_sbr_stream_init(p->sst, n);
        // the null header (table entry 0) is what frames before their stream's first header point at
        ok = hipMemcpy(p->d_hdr, heaac_sbr_table_data(p->tab), sizeof(HeaacSbrHeader), hipMemcpyHostToDevice) == hipSuccess;
        p->hdr_uploaded = 1;
    }
    if (ok) {
        if (threads <= 0) threads = heaac_threads_by_cpu_quota();
        if (threads < 1) threads = 1;
        if (threads > 256) threads = 256;
        if ((size_t)threads > n) threads = (int)n;
        ok = (p->pool = heaac_pool_create(threads, pl_slice, p)) != NULL;
        if (ok) p->threads = heaac_pool_threads(p->pool);
    }
    if (!ok) { heaac_pipeline_destroy(p); return HEAAC_ERR_NOMEM; }
    *out = p;
    return HEAAC_OK;
}

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// GPU stage and D2H of the tick in set s, behind its in_done
static int pl_submit_rest(HeaacPipeline *p, Set *s)
{
    const size_t n = p->n, nf = p->nf;
    // GPU
    HIP_OK(hipStreamWaitEvent(p->run, s->in_done, 0));
    if (s->used) HIP_OK(hipStreamWaitEvent(p->run, s->out_done, 0));
    // a tick without a failed unit -- the usual one -- runs the plain kernels (NULL: no mask)
    const uint8_t *hold_dsp = s->any_held ? s->d_hold : NULL, *hold_tools = s->any_held ? s->d_hold + nf : NULL;
    int rc = heaac_spectral_tools_streams_ex(p->dev, p->ncore, s->d.coeffs, s->d.tools, p->d_rng, p->d_rng, p->d_pred,
                                             p->d_pred, n, p->T, hold_tools, (void *)p->run);
    if (rc == HEAAC_OK)
        rc = p->he ? heaac_he_decode_streams_ex(p->dev, p->he_cfg, p->downsampled ? HEAAC_HE_DOWNSAMPLED : 0, s->d.coeffs,
                                                s->d.ics, s->d.sbr, p->d_hdr, PL_MAX_HDRS, s->d.ps, p->d_state, p->d_state,
                                                s->d_pcm, HEAAC_PCM_S16_INTERLEAVED, n, p->T, hold_dsp, (void *)p->run)
                   : heaac_lc_decode_streams_ex(p->dev, p->ncore, s->d.coeffs, s->d.ics, p->d_state, p->d_state, s->d_pcm,
                                                HEAAC_PCM_S16_INTERLEAVED, n, p->T, hold_dsp, (void *)p->run);
    if (rc != HEAAC_OK) return rc;
    HIP_OK(hipEventRecord(s->run_done, p->run));
    // D2H
    HIP_OK(hipStreamWaitEvent(p->out, s->run_done, 0));
    HIP_OK(hipMemcpyAsync(s->h_pcm, s->d_pcm, nf * (size_t)p->nout * p->out_len * 2, hipMemcpyDeviceToHost, p->out));
    HIP_OK(hipEventRecord(s->out_done, p->out));
    s->used = 1;
    p->submitted++;
    return HEAAC_OK;
}

// A buffer pair of `have` bytes or units that must hold `needed`: the capacity to allocate, doubled from `first`
static size_t pl_grown(size_t needed, size_t have, size_t first, size_t most)
{
    size_t cap = have ? have : first;
    while (cap < needed) cap *= 2;
    return cap > most ? most : cap;
}

// The staging area for `units` units.  Nothing of the old one is in flight: the caller has waited for stg.done.
static int stg_grow(HeaacPipeline *p, size_t units)
{
    Staging *g = &p->stg;
    if (units <= g->cap) return HEAAC_OK;
    const size_t cap = pl_grown(units, g->cap, 64, p->nf);
    stg_free(g);
    if (!(rec_alloc(p, &g->mem, &g->h, &g->d, cap) && heaac_pair(&g->mem, &g->h_hold, &g->d_hold, 2 * cap) &&
          heaac_pair(&g->mem, &g->h_dest, &g->d_dest, cap * sizeof(uint32_t)))) {
        stg_free(g);
        return HEAAC_ERR_NOMEM;
    }
    g->cap = cap;
    return HEAAC_OK;
}

// The fix-up of a device-parse tick: the p->m streams the walk stopped (h_list, stop_base) are finished by the host
// parser from their gathered states, and what it made is scattered into the tick's rows; all on `in`.
// *held: some unit of the tick is held.
static int pl_fix_up(HeaacPipeline *p, Set *s, int *held)
{
    Staging *g = &p->stg;
    const size_t m = p->m, units = p->stop_base[m];
    int rc = stg_grow(p, units);
    if (rc != HEAAC_OK) return rc;
    HeaacSbrStream *d_sst = p->he ? p->d_sst[p->sst_cur] : NULL;
    // gather
    HIP_OK(hipMemcpyAsync(p->d_list, p->h_list, m * sizeof(uint32_t), hipMemcpyHostToDevice, p->in));
    rc = heaac_launch_fix_gather(p->in, p->d_list, m, p->d_ast, p->m_g_ast, d_sst, p->m_g_sst);
    if (rc != HEAAC_OK) return rc;
    HIP_OK(hipStreamSynchronize(p->in));
    // host parse
    heaac_pool_run(p->pool, 2);
    *held = memchr(g->h_hold, 1, units) != NULL;
    // new SBR headers of this tick (the table's storage never moves)
    if (heaac_sbr_table_count(p->tab) > PL_MAX_HDRS) return HEAAC_ERR_ARG;
    rc = heaac_upload_headers(p->tab, &p->hdr_uploaded, p->d_hdr, NULL, p->in);
    if (rc != HEAAC_OK) return rc;
    // scatter
    rc = rec_upload(p, &g->h, &g->d, units, false);
    if (rc != HEAAC_OK) return rc;
    HIP_OK(hipMemcpyAsync(g->d_hold, g->h_hold, 2 * units, hipMemcpyHostToDevice, p->in));
    HIP_OK(hipMemcpyAsync(g->d_dest, g->h_dest, units * sizeof(uint32_t), hipMemcpyHostToDevice, p->in));
    HIP_OK(hipMemcpyAsync(p->d_g_ast, p->h_g_ast, m * sizeof(HeaacAacStream), hipMemcpyHostToDevice, p->in));
    if (p->he) HIP_OK(hipMemcpyAsync(p->d_g_sst, p->h_g_sst, m * sizeof(HeaacSbrStream), hipMemcpyHostToDevice, p->in));
    HeaacFixRows rows;
    memset(&rows, 0, sizeof(rows));
    for (int k = 0; k < HEAAC_FIX_ARRAYS; k++) {
        rows.dst[k] = (uint32_t *)s->d.row[k]; rows.src[k] = (const uint32_t *)g->d.row[k];
        rows.words[k] = (uint32_t)(p->row_bytes[k] / 4);
    }
    rc = heaac_launch_fix_scatter(p->in, &rows, g->d_dest, units, g->d_hold, s->d_hold, p->nf, p->d_list, m, p->d_g_ast, p->d_ast,
                                  p->d_g_sst, d_sst);
    if (rc != HEAAC_OK) return rc;
    HIP_OK(hipEventRecord(g->done, p->in));
    g->used = 1;
    return HEAAC_OK;
}

// The first two stages of a device-parse tick, up to in_done: pack, upload, the walk and the status kernel on `in`,
// the wait for the stop positions, the fix-up.  (The set's pinned inputs are free: submit has waited for in_done.)
static int pl_submit_device(HeaacPipeline *p, Set *s, const uint8_t *const *au, const int *size, int *status, double t0)
{
    const size_t n = p->n, nf = p->nf;
    // pack
    if (heaac_pack_offsets(size, nf, s->h_off) != 0) return HEAAC_ERR_ARG;
    const size_t total = s->h_off[nf];
    if (total > s->bytes_cap || !s->bytes_cap) {
        // (the walk that read the old buffer has finished: every submit waits for its own)
        const size_t cap = pl_grown(total, s->bytes_cap, 1 << 16, (size_t)1 << 32);
        if (s->h_bytes) (void)hipHostFree(s->h_bytes);
        if (s->d_bytes) (void)hipFree(s->d_bytes);
        s->h_bytes = NULL; s->d_bytes = NULL; s->bytes_cap = 0;
        if (!pinned((void **)&s->h_bytes, cap) || !devmem((void **)&s->d_bytes, cap)) return HEAAC_ERR_NOMEM;
        s->bytes_cap = cap;
    }
    p->job_au = au; p->job_size = size; p->job_status = status; p->job_set = s;
    heaac_pool_run(p->pool, 1);
    // upload
    if (s->used) HIP_OK(hipStreamWaitEvent(p->in, s->run_done, 0));
    HIP_OK(hipEventRecord(s->in_start, p->in));
    if (total) HIP_OK(hipMemcpyAsync(s->d_bytes, s->h_bytes, total, hipMemcpyHostToDevice, p->in));
    HIP_OK(hipMemcpyAsync(s->d_off, s->h_off, (nf + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, p->in));
    // parse: the walk, then the statuses of the host parser
    int rc;
    if (p->he) {
        rc = heaac_heaac_parse_device_streams(p->dev, &p->aac, p->d_ast, p->d_sst[p->sst_cur], p->d_sst[p->sst_cur ^ 1], s->d_bytes,
                                              s->d_off, n, p->T, p->ncore, s->d.coeffs, s->d.ics, s->d.tools, p->d_info, p->d_hdr,
                                              p->hdr_uploaded, s->d.sbr, s->d.ps, p->d_status, p->m_taken, s->d_hold, (void *)p->in);
        if (rc == HEAAC_OK) p->sst_cur ^= 1;
    } else {
        rc = heaac_aac_parse_device_streams(p->dev, &p->aac, p->d_ast, s->d_bytes, s->d_off, n, p->T, p->ncore, s->d.coeffs,
                                            s->d.ics, s->d.tools, p->d_info, p->d_status, p->m_taken, s->d_hold, (void *)p->in);
    }
    if (rc == HEAAC_OK)
        rc = heaac_launch_parse_status(p->in, p->d_status, p->d_info, p->he, p->aac.sbr == 0, status ? p->m_status : NULL,
                                       s->d_hold + nf, nf);
    if (rc != HEAAC_OK) return rc;
    HIP_OK(hipEventRecord(p->parsed, p->in));
    // the staging area and the stop list are free once the scatter of the tick that used them last has run
    if (p->stg.used) HIP_OK(hipEventSynchronize(p->stg.done));
    HIP_OK(hipEventSynchronize(p->parsed));
    if (status) memcpy(status, p->h_status, nf * sizeof(int32_t));
    p->m = heaac_stop_list(p->h_taken, n, (uint32_t)p->T, p->h_list, p->stop_base);
    p->n_host += p->stop_base[p->m];
    p->n_device += nf - p->stop_base[p->m];
    int held = 0;
    if (p->m) {
        rc = pl_fix_up(p, s, &held);
        if (rc != HEAAC_OK) return rc;
    }
    s->any_held = held;
    HIP_OK(hipEventRecord(s->in_done, p->in));
    s->parse_ms = (float)(now_ms() - t0);
    return HEAAC_OK;
}

// The first two stages of a host-parse tick, up to in_done: the parser pool, then the records and the masks on `in`
static int pl_submit_host(HeaacPipeline *p, Set *s, const uint8_t *const *au, const int *size, int *status, double t0)
{
    const size_t nf = p->nf;
    p->job_au = au; p->job_size = size; p->job_status = status; p->job_set = s;
    heaac_pool_run(p->pool, 0);
    s->parse_ms = (float)(now_ms() - t0);
    // new SBR headers of this tick (the table's storage never moves)
    if (heaac_sbr_table_count(p->tab) > PL_MAX_HDRS) return HEAAC_ERR_ARG;
    // H2D
    if (s->used) HIP_OK(hipStreamWaitEvent(p->in, s->run_done, 0));
    HIP_OK(hipEventRecord(s->in_start, p->in));
    int rc = heaac_upload_headers(p->tab, &p->hdr_uploaded, p->d_hdr, NULL, p->in);
    if (rc == HEAAC_OK) rc = rec_upload(p, &s->h, &s->d, nf, p->ncore == 1);
    if (rc != HEAAC_OK) return rc;
    s->any_held = memchr(s->h_hold, 1, nf) != NULL;
    if (s->any_held) HIP_OK(hipMemcpyAsync(s->d_hold, s->h_hold, 2 * nf, hipMemcpyHostToDevice, p->in));
    HIP_OK(hipEventRecord(s->in_done, p->in));
    p->n_host += nf;
    return HEAAC_OK;
}

extern "C" int heaac_pipeline_submit(HeaacPipeline *p, const uint8_t *const *au, const int *size, int *status)
{
    if (!p || !au || !size) return HEAAC_ERR_ARG;
    if (p->submitted - p->collected >= PL_DEPTH) return HEAAC_ERR_ARG;
    Set *s = &p->set[p->submitted % PL_DEPTH];
    // the pinned inputs of this set are free once the H2D of the tick that used it last has finished
    if (s->used) HIP_OK(hipEventSynchronize(s->in_done));
    const double t0 = now_ms();
    const int rc = p->dp ? pl_submit_device(p, s, au, size, status, t0) : pl_submit_host(p, s, au, size, status, t0);
    return rc != HEAAC_OK ? rc : pl_submit_rest(p, s);
}

extern "C" int heaac_pipeline_collect(HeaacPipeline *p, const int16_t **pcm)
{
    if (!p || !pcm || p->collected == p->submitted) return HEAAC_ERR_ARG;
    Set *s = &p->set[p->collected % PL_DEPTH];
    HIP_OK(hipEventSynchronize(s->out_done));
    *pcm = s->h_pcm;
    p->last_ms[0] = s->parse_ms;
    (void)hipEventElapsedTime(&p->last_ms[1], s->in_start, s->in_done);
    (void)hipEventElapsedTime(&p->last_ms[2], s->in_done, s->run_done);
    (void)hipEventElapsedTime(&p->last_ms[3], s->run_done, s->out_done);
    p->collected++;
    return HEAAC_OK;
}

extern "C" void heaac_pipeline_timing(const HeaacPipeline *p, float ms[4])
{
    for (int k = 0; k < 4; k++) ms[k] = p ? p->last_ms[k] : 0.0f;
}

// ---- include/heaac_debug.h: the two plain-C steps of a device-parse tick (pipeline_pack.h) ----
extern "C" int heaac_debug_pipeline_pack(const uint8_t *const *au, const int *size, size_t n_units, uint8_t *bytes,
                                         uint32_t *offset)
{
    if (!size || !offset) return HEAAC_ERR_ARG;
    if (heaac_pack_offsets(size, n_units, offset) != 0) return HEAAC_ERR_ARG;
    if (bytes) {
        if (!au) return HEAAC_ERR_ARG;
        heaac_pack_bytes(au, size, offset, 0, n_units, bytes);
    }
    return HEAAC_OK;
}

extern "C" size_t heaac_debug_pipeline_stops(const uint32_t *taken, size_t n_streams, size_t frames_per_tick, uint32_t *list,
                                             uint32_t *base)
{
    if (!taken || !list || !base || frames_per_tick > 0xffffffffull) return 0;
    return heaac_stop_list(taken, n_streams, (uint32_t)frames_per_tick, list, base);
}
