// capi.hip -- the C ABI of include/heaac_dsp.h: device context + entry points.
//
// Thin by design: argument checks, table upload, kernel launches.  No host
// fallback exists -- if no HIP device is usable every entry point fails with
// HEAAC_ERR_NODEVICE / HEAAC_ERR_HIP.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "heaac_dsp.h"
#include "heaac_debug.h"
#include "heaac_parse.h"
#include "parse_core.h"
#include "sbr_core.h"
#include "parse_streams.h"
#include "tables.h"
#include "kernels.h"
#include "host_common.h"

#define HE_MAX_LANES 4
#define HE_ZERO_BYTES (2 * 38 * 64 * 4)      // one channel's X record of +0: what k_synth reads for bands that were not stored
struct HeaacDevice {
    int device;
    float *d_tab;
    uint16_t *d_rev;
    HeaacParseTables *d_ptab;   // parse_core.h: what heaac_aac_parse_device reads (code trees, dequantisation and band tables)
    HeaacSbrParseTables *d_stab;    // sbr_core.h: the SBR / PS code books heaac_sbr_parse_device reads
    void *d_work;
    unsigned *d_queue;      // frame-queue heads of the kernels that draw frames dynamically (one set per lane)
    // X hand-over side data: a page of zeros, then per workspace set one byte per frame and channel = the number of QMF
    // bands of the X rows the HF / PS stage has stored (the bands above are +0 and are not written; the synthesis
    // kernel reads them from the zero page instead)
    unsigned char *d_aux;
    size_t work_bytes;
    size_t max_frames;
    size_t chunk;
    int sets;               // workspace sets allocated: 1 (batches of one chunk) or HE_LANES
    // Chunks of one HE call alternate between two internal streams ("lanes"), each with its own
    // workspace half and queue heads: the persistent kernels of one chunk drain while the next
    // chunk's kernels fill the freed CUs, so a chunk can be small enough for its W / X workspace to
    // live in the 256 MiB Infinity Cache between the kernel that writes it and the one that reads it.
    hipStream_t lane[HE_MAX_LANES];
    hipEvent_t fork, join[HE_MAX_LANES];
    int lanes;
    // The HE calls share the workspace and the queue heads, so they must not overlap: the stream of the
    // last HE call and an event behind its launches are kept, and a call that arrives on ANOTHER stream
    // while that work is still in flight is refused (HEAAC_ERR_ARG) instead of racing on the workspace.
    hipStream_t owner;
    hipEvent_t done;
    int owner_valid, done_recorded;
};

// Claim the HE workspace for stream s (see HeaacDevice::owner).
static int he_claim(HeaacDevice *d, hipStream_t s, bool *capturing)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    *capturing = cs != hipStreamCaptureStatusNone;
    if (d->owner_valid && d->owner != s) {
        // the earlier call's work must have finished; inside a capture that cannot be asked
        if (*capturing) return HEAAC_ERR_ARG;
        if (d->done_recorded) {
            const hipError_t q = hipEventQuery(d->done);
            if (q == hipErrorNotReady) return HEAAC_ERR_ARG;
            if (q != hipSuccess) { (void)hipGetLastError(); return HEAAC_ERR_HIP; }
        }
    }
    d->owner = s;
    d->owner_valid = 1;
    return HEAAC_OK;
}
static int he_release(HeaacDevice *d, hipStream_t s, bool capturing, int rc)
{
    d->done_recorded = 0;
    if (!capturing) {
        if (hipEventRecord(d->done, s) != hipSuccess) return rc == HEAAC_OK ? HEAAC_ERR_HIP : rc;
        d->done_recorded = 1;
    }
    return rc;
}
static int he_lanes()
{
    int l = 2;
#ifdef HEAAC_TUNING
    const char *env = getenv("HEAAC_LANES");                 /* -DHEAAC_TUNING builds only: lanes sweep */
    if (env) l = atoi(env);
#endif
    return l < 1 ? 1 : l > HE_MAX_LANES ? HE_MAX_LANES : l;
}
#define HE_LANES he_lanes()

static bool pcm_format_ok(int f)
{
    return f == HEAAC_PCM_F32_PLANAR || f == HEAAC_PCM_S16_INTERLEAVED || f == HEAAC_PCM_S16_INTERLEAVED_SSE2;
}
static bool he_cfg_ok(int cfg) { return heaac_cfg_shape(cfg).he != 0; }

extern "C" const char *heaac_build_info(void)
{
    return "heaac-amd gfx950 (hipcc, -ffp-contract=off) " __DATE__ " " __TIME__;
}

extern "C" const char *heaac_strerror(int err)
{
    switch (err) {
    case HEAAC_OK: return "ok";
    case HEAAC_ERR_ARG: return "bad argument or unsupported configuration";
    case HEAAC_ERR_HIP: return "HIP runtime error";
    case HEAAC_ERR_NOMEM: return "out of memory";
    case HEAAC_ERR_NODEVICE: return "no usable gfx950 device";
    }
    return "unknown error";
}

// HE pipeline stages exchange W[ncore][32][32][2] and X[2][2][38][64] per frame through this
// workspace, one chunk of frames at a time.  Measured on MI355X (profiles/r01_chunk_sweep.txt,
// profiles/r02_chunk_lanes.txt): throughput rises with the chunk size (the tails of the persistent
// kernels amortise) up to the whole 256 k-frame batch; chunks small enough to keep the workspace
// in the 256 MiB Infinity Cache lose more in tails than they save, also when consecutive chunks
// overlap on two streams.  Batches beyond one chunk alternate between two lanes (below).
#define HE_CHUNK_FRAMES 262144
#define WS_W_FLOATS (2 * 2048)
#define WS_X_FLOATS (2 * 2 * 38 * 64)

static size_t he_chunk_frames(size_t max_frames)
{
    size_t cap = HE_CHUNK_FRAMES;
#ifdef HEAAC_TUNING
    const char *env = getenv("HEAAC_CHUNK_FRAMES");          /* -DHEAAC_TUNING builds only: chunk sweep */
    if (env && atol(env) >= 64) cap = (size_t)atol(env);
#endif
    size_t chunk = max_frames < cap ? max_frames : cap;
    return chunk < 64 ? 64 : chunk;
}

// one workspace set per lane, at most one per chunk; a batch that fits one chunk runs on the caller's stream alone
static size_t he_sets(size_t max_frames)
{
    const size_t chunk = he_chunk_frames(max_frames), chunks = (max_frames + chunk - 1) / chunk;
    const size_t lanes = (size_t)HE_LANES;
    return chunks <= 1 ? 1 : chunks < lanes ? chunks : lanes;
}

extern "C" size_t heaac_device_workspace_bytes(size_t max_frames)
{
    return he_sets(max_frames) * he_chunk_frames(max_frames) * (WS_W_FLOATS + WS_X_FLOATS) * sizeof(float);
}

extern "C" int heaac_device_create(HeaacDevice **out, size_t max_frames)
{
    if (!out) return HEAAC_ERR_ARG;
    *out = NULL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return HEAAC_ERR_NODEVICE;
    HeaacDevice *d = (HeaacDevice *)calloc(1, sizeof(*d));
    if (!d) return HEAAC_ERR_NOMEM;
    if (hipGetDevice(&d->device) != hipSuccess) { free(d); return HEAAC_ERR_HIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) != hipSuccess ||
        strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        free(d);
        return HEAAC_ERR_NODEVICE;
    }
    HeaacHostTables *t = (HeaacHostTables *)malloc(sizeof(*t));
    if (!t) { free(d); return HEAAC_ERR_NOMEM; }
    heaac_build_tables(t);
    d->max_frames = max_frames;
    d->work_bytes = heaac_device_workspace_bytes(max_frames);
    d->chunk = he_chunk_frames(max_frames);
    d->sets = (int)he_sets(max_frames);
    int rc = HEAAC_OK;
    if (hipMalloc((void **)&d->d_tab, sizeof(t->f)) != hipSuccess ||
        hipMalloc((void **)&d->d_rev, sizeof(t->rev)) != hipSuccess ||
        hipMalloc((void **)&d->d_queue, 64 * HE_MAX_LANES) != hipSuccess ||
        hipMalloc((void **)&d->d_aux, HE_ZERO_BYTES + 2 * (size_t)(d->sets > 0 ? d->sets : 1) * (d->chunk ? d->chunk : 1)) != hipSuccess ||
        hipMalloc((void **)&d->d_ptab, sizeof(HeaacParseTables)) != hipSuccess ||
        hipMalloc((void **)&d->d_stab, sizeof(HeaacSbrParseTables)) != hipSuccess ||
        (d->work_bytes && hipMalloc(&d->d_work, d->work_bytes) != hipSuccess))
        rc = HEAAC_ERR_NOMEM;
    const HeaacParseTables *pt = heaac_parse_tables();
    if (rc == HEAAC_OK && (!pt || hipMemcpy(d->d_ptab, pt, sizeof(*pt), hipMemcpyHostToDevice) != hipSuccess))
        rc = HEAAC_ERR_HIP;
    const HeaacSbrParseTables *spt = heaac_sbr_parse_tables();
    if (rc == HEAAC_OK && (!spt || hipMemcpy(d->d_stab, spt, sizeof(*spt), hipMemcpyHostToDevice) != hipSuccess))
        rc = HEAAC_ERR_HIP;
    if (rc == HEAAC_OK &&
        (hipMemset(d->d_aux, 0, HE_ZERO_BYTES) != hipSuccess ||
         hipMemcpy(d->d_tab, t->f, sizeof(t->f), hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(d->d_rev, t->rev, sizeof(t->rev), hipMemcpyHostToDevice) != hipSuccess))
        rc = HEAAC_ERR_HIP;
    free(t);
    d->lanes = HE_LANES;
    if (rc == HEAAC_OK && (hipEventCreateWithFlags(&d->fork, hipEventDisableTiming) != hipSuccess ||
                           hipEventCreateWithFlags(&d->done, hipEventDisableTiming) != hipSuccess))
        rc = HEAAC_ERR_HIP;
    for (int k = 0; k < d->lanes && rc == HEAAC_OK; k++)
        if (hipEventCreateWithFlags(&d->join[k], hipEventDisableTiming) != hipSuccess ||
            hipStreamCreateWithFlags(&d->lane[k], hipStreamNonBlocking) != hipSuccess)
            rc = HEAAC_ERR_HIP;
    if (rc != HEAAC_OK) {
        heaac_device_destroy(d);
        return rc;
    }
    *out = d;
    return HEAAC_OK;
}

extern "C" void heaac_device_destroy(HeaacDevice *d)
{
    if (!d) return;
    if (d->d_tab) (void)hipFree(d->d_tab);
    if (d->d_rev) (void)hipFree(d->d_rev);
    if (d->d_ptab) (void)hipFree(d->d_ptab);
    if (d->d_stab) (void)hipFree(d->d_stab);
    if (d->d_work) (void)hipFree(d->d_work);
    if (d->d_queue) (void)hipFree(d->d_queue);
    if (d->d_aux) (void)hipFree(d->d_aux);
    for (int k = 0; k < HE_MAX_LANES; k++) {
        if (d->lane[k]) (void)hipStreamDestroy(d->lane[k]);
        if (d->join[k]) (void)hipEventDestroy(d->join[k]);
    }
    if (d->fork) (void)hipEventDestroy(d->fork);
    if (d->done) (void)hipEventDestroy(d->done);
    free(d);
}

extern "C" int heaac_imdct_half_batch(HeaacDevice *dev, int which, float *d_out, const float *d_in,
                                      size_t n, void *stream)
{
    if (!dev || which < 0 || which > 3)
        return HEAAC_ERR_ARG;
    if (n == 0)
        return HEAAC_OK;
    if (!d_out || !d_in || d_out == d_in)
        return HEAAC_ERR_ARG;
    return heaac_launch_imdct_half(dev->d_tab, dev->d_rev, which, d_out, d_in, n, (hipStream_t)stream);
}

extern "C" int heaac_lc_decode_batch(HeaacDevice *dev, int channels,
                                     const float *d_coeffs, const HeaacIcs *d_ics,
                                     const float *d_state_in, float *d_state_out,
                                     void *d_pcm, int pcm_format, size_t n, void *stream)
{
    if (!dev || channels < 1 || channels > 2 || !pcm_format_ok(pcm_format))
        return HEAAC_ERR_ARG;
    if (n == 0)
        return HEAAC_OK;
    if (!d_coeffs || !d_ics || !d_state_in || !d_state_out || !d_pcm)
        return HEAAC_ERR_ARG;
    return heaac_launch_lc(dev->d_tab, dev->d_rev, channels, d_coeffs, d_ics, d_state_in, d_state_out,
                           d_pcm, pcm_format, n, 1, NULL, (hipStream_t)stream);
}

extern "C" int heaac_lc_decode_streams(HeaacDevice *dev, int channels,
                                       const float *d_coeffs, const HeaacIcs *d_ics,
                                       const float *d_state_in, float *d_state_out,
                                       void *d_pcm, int pcm_format,
                                       size_t n_streams, size_t frames_per_stream, void *stream)
{
    return heaac_lc_decode_streams_ex(dev, channels, d_coeffs, d_ics, d_state_in, d_state_out, d_pcm, pcm_format,
                                      n_streams, frames_per_stream, NULL, stream);
}

extern "C" int heaac_lc_decode_streams_ex(HeaacDevice *dev, int channels,
                                          const float *d_coeffs, const HeaacIcs *d_ics,
                                          const float *d_state_in, float *d_state_out,
                                          void *d_pcm, int pcm_format,
                                          size_t n_streams, size_t frames_per_stream,
                                          const uint8_t *d_hold, void *stream)
{
    if (!dev || channels < 1 || channels > 2 || !pcm_format_ok(pcm_format) || frames_per_stream == 0)
        return HEAAC_ERR_ARG;
    if (n_streams == 0)
        return HEAAC_OK;
    if (!d_coeffs || !d_ics || !d_state_in || !d_state_out || !d_pcm)
        return HEAAC_ERR_ARG;
    // S * T frames of channels x 1024 floats must be addressable
    const size_t frame_bytes = (size_t)channels * 1024 * sizeof(float);
    if (n_streams > SIZE_MAX / frames_per_stream || n_streams * frames_per_stream > SIZE_MAX / frame_bytes)
        return HEAAC_ERR_ARG;
    return heaac_launch_lc(dev->d_tab, dev->d_rev, channels, d_coeffs, d_ics, d_state_in, d_state_out,
                           d_pcm, pcm_format, n_streams, frames_per_stream, d_hold, (hipStream_t)stream);
}

extern "C" int heaac_aac_parse_device(HeaacDevice *dev, const HeaacAacConfig *cfg, HeaacAacStream *d_st,
                                      const uint8_t *d_au, const uint32_t *d_au_offset, size_t n, int coeff_channels,
                                      float *d_coeffs, HeaacIcs *d_ics, HeaacToolsFrame *d_tools,
                                      HeaacAacFrameInfo *d_info, int32_t *d_status, void *stream)
{
    if (!dev || !heaac_parse_args_ok(cfg, coeff_channels))
        return HEAAC_ERR_ARG;
    if (n == 0)
        return HEAAC_OK;
    // the walk stores a quad codeword's four lines as one 16-byte word
    if (!d_st || !d_au || !d_au_offset || !d_coeffs || !d_ics || !d_tools || !d_info || !d_status ||
        ((uintptr_t)d_coeffs & 15) || ((uintptr_t)d_tools & 3) || ((uintptr_t)d_au_offset & 3) || ((uintptr_t)d_info & 3) || ((uintptr_t)d_status & 3))
        return HEAAC_ERR_ARG;
    return heaac_launch_aac_parse(dev->d_ptab, cfg, d_st, d_au, d_au_offset, n, coeff_channels, d_coeffs, d_ics, d_tools,
                                  d_info, d_status, (hipStream_t)stream);
}

extern "C" int heaac_sbr_parse_device(HeaacDevice *dev, const HeaacAacConfig *cfg, const HeaacSbrStream *d_sst_in,
                                      HeaacSbrStream *d_sst_out, const uint8_t *d_au, const uint32_t *d_au_offset,
                                      const HeaacAacFrameInfo *d_info, const int32_t *d_aac_status, size_t n,
                                      const HeaacSbrHeader *d_hdr, size_t n_hdr, HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps,
                                      int32_t *d_status, void *stream)
{
    if (!dev || !cfg)
        return HEAAC_ERR_ARG;
    if (n == 0)
        return HEAAC_OK;
    if (n > PARSE_GRID_MAX || ((uintptr_t)d_aac_status & 3) ||
        !heaac_sbr_parse_args_ok(cfg, d_sst_in, d_sst_out, d_au, d_au_offset, d_info, n, d_hdr, n_hdr, d_sbr, d_ps, d_status))
        return HEAAC_ERR_ARG;
    return heaac_launch_sbr_parse(dev->d_stab, cfg, d_sst_in, d_sst_out, d_au, d_au_offset, d_info, d_aac_status, n, d_hdr, n_hdr,
                                  d_sbr, d_ps, d_status, (hipStream_t)stream);
}

extern "C" int heaac_heaac_parse_device(HeaacDevice *dev, const HeaacAacConfig *cfg, HeaacAacStream *d_st,
                                        const HeaacSbrStream *d_sst_in, HeaacSbrStream *d_sst_out, const uint8_t *d_au,
                                        const uint32_t *d_au_offset, size_t n, int coeff_channels, float *d_coeffs,
                                        HeaacIcs *d_ics, HeaacToolsFrame *d_tools, HeaacAacFrameInfo *d_info,
                                        const HeaacSbrHeader *d_hdr, size_t n_hdr, HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps,
                                        int32_t *d_status, void *stream)
{
    if (!dev || !heaac_parse_args_ok(cfg, coeff_channels))
        return HEAAC_ERR_ARG;
    if (n == 0)
        return HEAAC_OK;
    // everything either half refuses is refused before the first launch
    if (n > PARSE_GRID_MAX ||
        !heaac_sbr_parse_args_ok(cfg, d_sst_in, d_sst_out, d_au, d_au_offset, d_info, n, d_hdr, n_hdr, d_sbr, d_ps, d_status))
        return HEAAC_ERR_ARG;
    int rc = heaac_aac_parse_device(dev, cfg, d_st, d_au, d_au_offset, n, coeff_channels, d_coeffs, d_ics, d_tools, d_info, d_status,
                                    stream);
    if (rc != HEAAC_OK)
        return rc;
    // the SBR half reads each unit's AAC status from d_status and writes the unit's one status there
    return heaac_sbr_parse_device(dev, cfg, d_sst_in, d_sst_out, d_au, d_au_offset, d_info, d_status, n, d_hdr, n_hdr, d_sbr, d_ps,
                                  d_status, stream);
}

extern "C" int heaac_aac_parse_device_streams(HeaacDevice *dev, const HeaacAacConfig *cfg, HeaacAacStream *d_st, const uint8_t *d_au,
                                              const uint32_t *d_au_offset, size_t n_streams, size_t frames_per_stream,
                                              int coeff_channels, float *d_coeffs, HeaacIcs *d_ics, HeaacToolsFrame *d_tools,
                                              HeaacAacFrameInfo *d_info, int32_t *d_status, uint32_t *d_taken, uint8_t *d_hold,
                                              void *stream)
{
    if (!dev || !heaac_parse_args_ok(cfg, coeff_channels) || frames_per_stream == 0)
        return HEAAC_ERR_ARG;
    if (n_streams == 0)
        return HEAAC_OK;
    if (!heaac_parse_streams_args_ok(cfg, 0, d_st, NULL, NULL, d_au, d_au_offset, n_streams, frames_per_stream, d_coeffs, d_ics,
                                     d_tools, d_info, NULL, 0, NULL, NULL, d_status, d_taken))
        return HEAAC_ERR_ARG;
    return heaac_launch_parse_streams(dev->d_ptab, NULL, cfg, d_st, NULL, NULL, d_au, d_au_offset, n_streams, frames_per_stream,
                                      coeff_channels, d_coeffs, d_ics, d_tools, d_info, NULL, 0, NULL, NULL, d_status, d_taken, d_hold,
                                      (hipStream_t)stream);
}

extern "C" int heaac_heaac_parse_device_streams(HeaacDevice *dev, const HeaacAacConfig *cfg, HeaacAacStream *d_st,
                                                const HeaacSbrStream *d_sst_in, HeaacSbrStream *d_sst_out, const uint8_t *d_au,
                                                const uint32_t *d_au_offset, size_t n_streams, size_t frames_per_stream,
                                                int coeff_channels, float *d_coeffs, HeaacIcs *d_ics, HeaacToolsFrame *d_tools,
                                                HeaacAacFrameInfo *d_info, const HeaacSbrHeader *d_hdr, size_t n_hdr,
                                                HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps, int32_t *d_status, uint32_t *d_taken,
                                                uint8_t *d_hold, void *stream)
{
    if (!dev || !heaac_parse_args_ok(cfg, coeff_channels) || frames_per_stream == 0)
        return HEAAC_ERR_ARG;
    if (n_streams == 0)
        return HEAAC_OK;
    if (!heaac_parse_streams_args_ok(cfg, 1, d_st, d_sst_in, d_sst_out, d_au, d_au_offset, n_streams, frames_per_stream, d_coeffs,
                                     d_ics, d_tools, d_info, d_hdr, n_hdr, d_sbr, d_ps, d_status, d_taken))
        return HEAAC_ERR_ARG;
    return heaac_launch_parse_streams(dev->d_ptab, dev->d_stab, cfg, d_st, d_sst_in, d_sst_out, d_au, d_au_offset, n_streams,
                                      frames_per_stream, coeff_channels, d_coeffs, d_ics, d_tools, d_info, d_hdr, n_hdr, d_sbr, d_ps,
                                      d_status, d_taken, d_hold, (hipStream_t)stream);
}

extern "C" int heaac_spectral_tools_batch(HeaacDevice *dev, int channels, float *d_coeffs,
                                          const HeaacToolsFrame *d_tools,
                                          const int32_t *d_rng_in, int32_t *d_rng_out,
                                          const HeaacPredictorState *d_pred_in, HeaacPredictorState *d_pred_out,
                                          size_t n, void *stream)
{
    return heaac_spectral_tools_batch_ex(dev, channels, HEAAC_TOOLS_ALL, d_coeffs, d_tools, d_rng_in, d_rng_out,
                                         d_pred_in, d_pred_out, NULL, NULL, 0, n, stream);
}

extern "C" int heaac_spectral_tools_batch_ex(HeaacDevice *dev, int channels, int stages, float *d_coeffs,
                                             const HeaacToolsFrame *d_tools,
                                             const int32_t *d_rng_in, int32_t *d_rng_out,
                                             const HeaacPredictorState *d_pred_in, HeaacPredictorState *d_pred_out,
                                             const HeaacCceFrame *d_cce, const float *d_cce_coeffs, int n_cce,
                                             size_t n, void *stream)
{
    if (!dev || channels < 1 || channels > 2 || (d_rng_in && !d_rng_out) || (d_pred_in && !d_pred_out) ||
        !stages || (stages & ~HEAAC_TOOLS_ALL) || n_cce < 0 || n_cce > HEAAC_MAX_CCE ||
        (n_cce && (!d_cce || !d_cce_coeffs)))
        return HEAAC_ERR_ARG;
    if (n == 0)
        return HEAAC_OK;
    if (!d_coeffs || !d_tools)
        return HEAAC_ERR_ARG;
    return heaac_launch_spectral_tools(channels, d_coeffs, d_tools, d_rng_in, d_rng_out, d_pred_in, d_pred_out,
                                       stages, d_cce, d_cce_coeffs, n_cce, n, (hipStream_t)stream);
}

extern "C" int heaac_spectral_tools_streams(HeaacDevice *dev, int channels, float *d_coeffs,
                                            const HeaacToolsFrame *d_tools,
                                            const int32_t *d_rng_in, int32_t *d_rng_out,
                                            const HeaacPredictorState *d_pred_in, HeaacPredictorState *d_pred_out,
                                            size_t n_streams, size_t frames_per_stream, void *stream)
{
    return heaac_spectral_tools_streams_ex(dev, channels, d_coeffs, d_tools, d_rng_in, d_rng_out, d_pred_in, d_pred_out,
                                           n_streams, frames_per_stream, NULL, stream);
}

extern "C" int heaac_spectral_tools_streams_ex(HeaacDevice *dev, int channels, float *d_coeffs,
                                               const HeaacToolsFrame *d_tools,
                                               const int32_t *d_rng_in, int32_t *d_rng_out,
                                               const HeaacPredictorState *d_pred_in, HeaacPredictorState *d_pred_out,
                                               size_t n_streams, size_t frames_per_stream,
                                               const uint8_t *d_hold, void *stream)
{
    if (!dev || channels < 1 || channels > 2 || frames_per_stream == 0 || (d_rng_in && !d_rng_out) ||
        (d_pred_in && !d_pred_out))
        return HEAAC_ERR_ARG;
    if (n_streams == 0)
        return HEAAC_OK;
    if (!d_coeffs || !d_tools)
        return HEAAC_ERR_ARG;
    // S * T frames of coefficients and records must be addressable, and k_tns's grid (3 filters per channel, 256
    // lanes per block) must stay within its 2^31 - 1 blocks
    if (n_streams > SIZE_MAX / frames_per_stream)
        return HEAAC_ERR_ARG;
    const size_t n = n_streams * frames_per_stream;
    if (n > SIZE_MAX / ((size_t)channels * 1024 * sizeof(float)) || n > SIZE_MAX / sizeof(HeaacToolsFrame) ||
        n > 0x7fffffffull * 256 / (3 * (size_t)channels))
        return HEAAC_ERR_ARG;
    return heaac_launch_spectral_tools_streams(channels, d_coeffs, d_tools, d_rng_in, d_rng_out, d_pred_in,
                                               d_pred_out, n_streams, frames_per_stream, d_hold, (hipStream_t)stream);
}

// The HE calls behind their argument checks: n_streams streams of T consecutive frames each.  Whole streams per
// workspace set (a stream's T frames hand W / X over inside one set); with T = 1 a stream is a frame and the
// per-frame arrays and the state are exactly the batch call's (heaac_launch_he chooses the kernels).
static int he_walk(HeaacDevice *dev, int cfg, int flags, const float *d_coeffs, const HeaacIcs *d_ics,
                   const HeaacSbrFrame *d_sbr, const HeaacSbrHeader *d_hdr, size_t n_hdr, const HeaacPsFrame *d_ps,
                   const float *d_state_in, float *d_state_out, void *d_pcm, int pcm_format,
                   size_t n_streams, size_t T, const uint8_t *d_hold, hipStream_t s)
{
    const HeaacCfgShape shape = heaac_cfg_shape(cfg);
    const size_t ncore = shape.ncore, words = shape.words;
    const size_t pcm_bytes = (size_t)shape.nout * ((flags & HEAAC_HE_DOWNSAMPLED) ? 1024 : 2048) *
                             (pcm_format == HEAAC_PCM_F32_PLANAR ? 4 : 2);
    const size_t set_floats = dev->chunk * (WS_W_FLOATS + WS_X_FLOATS);
    const size_t per_chunk = dev->chunk / T;
    const unsigned hdrs = (unsigned)(n_hdr > 0xffffu ? 0x10000u : n_hdr);
    bool capturing = false;
    const int claim = he_claim(dev, s, &capturing);
    if (claim != HEAAC_OK) return claim;
    // one chunk: everything on the caller's stream; more: fork onto the two lanes and join again
    // (event fork / join, so the call stays capturable into a hipGraph)
    const bool lanes = n_streams > per_chunk && dev->sets > 1;
    const int nl = lanes ? dev->sets : 1;
    // (every exit behind he_claim goes through the join and he_release below: a failed fork must not leave the
    // workspace claimed or lanes that were already forked unjoined)
    int rc = HEAAC_OK;
    int forked = 0;
    if (lanes) {
        if (hipEventRecord(dev->fork, s) != hipSuccess) rc = HEAAC_ERR_HIP;
        for (int k = 0; k < nl && rc == HEAAC_OK; k++) {
            if (hipStreamWaitEvent(dev->lane[k], dev->fork, 0) != hipSuccess) rc = HEAAC_ERR_HIP;
            else forked = k + 1;
        }
    }
    HeaacHeLaunch a = {};
    a.d_tab = dev->d_tab; a.d_rev = dev->d_rev; a.cfg = cfg; a.flags = flags; a.d_hdr = d_hdr; a.n_hdr = hdrs;
    a.pcm_format = pcm_format; a.d_zero = (const float *)dev->d_aux; a.T = T;
    size_t c = 0;
    for (size_t s0 = 0; s0 < n_streams && rc == HEAAC_OK; s0 += per_chunk, c++) {
        const size_t f0 = s0 * T;
        const int k = (int)(c % nl);
        a.n_streams = n_streams - s0 < per_chunk ? n_streams - s0 : per_chunk;
        a.d_coeffs = d_coeffs + f0 * ncore * 1024; a.d_ics = d_ics + f0 * ncore; a.d_sbr = d_sbr + f0;
        a.d_ps = d_ps ? d_ps + f0 : NULL; a.d_hold = d_hold ? d_hold + f0 : NULL;
        a.d_state_in = d_state_in + s0 * words; a.d_state_out = d_state_out + s0 * words;
        a.d_pcm = (char *)d_pcm + f0 * pcm_bytes;
        a.d_ws_W = (float *)dev->d_work + k * set_floats; a.d_ws_X = a.d_ws_W + dev->chunk * WS_W_FLOATS;
        a.d_queue = dev->d_queue + 16 * k; a.d_xtop = dev->d_aux + HE_ZERO_BYTES + 2 * (size_t)k * dev->chunk;
        a.s = lanes ? dev->lane[k] : s;
        rc = heaac_launch_he(&a);
    }
    if (lanes) {
        // always rejoin, also after a failed launch (a capture must not be left forked)
        for (int k = 0; k < forked; k++)
            if (hipEventRecord(dev->join[k], dev->lane[k]) != hipSuccess ||
                hipStreamWaitEvent(s, dev->join[k], 0) != hipSuccess)
                rc = rc == HEAAC_OK ? HEAAC_ERR_HIP : rc;
    }
    return he_release(dev, s, capturing, rc);
}

extern "C" int heaac_he_decode_batch_ex(HeaacDevice *dev, int cfg, int flags,
                                     const float *d_coeffs, const HeaacIcs *d_ics,
                                     const HeaacSbrFrame *d_sbr,
                                     const HeaacSbrHeader *d_hdr, size_t n_hdr,
                                     const HeaacPsFrame *d_ps,
                                     const float *d_state_in, float *d_state_out,
                                     void *d_pcm, int pcm_format,
                                     size_t n, void *stream)
{
    if (!dev || !he_cfg_ok(cfg) || !pcm_format_ok(pcm_format) || (flags & ~HEAAC_HE_DOWNSAMPLED))
        return HEAAC_ERR_ARG;
    if (n == 0)
        return HEAAC_OK;
    if (!d_coeffs || !d_ics || !d_sbr || !d_hdr || !n_hdr || !d_state_in || !d_state_out || !d_pcm ||
        (cfg == HEAAC_CFG_HEV2 && !d_ps))
        return HEAAC_ERR_ARG;
    return he_walk(dev, cfg, flags, d_coeffs, d_ics, d_sbr, d_hdr, n_hdr, d_ps, d_state_in, d_state_out, d_pcm,
                   pcm_format, n, 1, NULL, (hipStream_t)stream);
}

extern "C" int heaac_he_decode_batch(HeaacDevice *dev, int cfg,
                                     const float *d_coeffs, const HeaacIcs *d_ics,
                                     const HeaacSbrFrame *d_sbr,
                                     const HeaacSbrHeader *d_hdr, size_t n_hdr,
                                     const HeaacPsFrame *d_ps,
                                     const float *d_state_in, float *d_state_out,
                                     void *d_pcm, int pcm_format,
                                     size_t n, void *stream)
{
    return heaac_he_decode_batch_ex(dev, cfg, 0, d_coeffs, d_ics, d_sbr, d_hdr, n_hdr, d_ps, d_state_in, d_state_out,
                                    d_pcm, pcm_format, n, stream);
}

extern "C" int heaac_he_decode_streams(HeaacDevice *dev, int cfg, int flags,
                                       const float *d_coeffs, const HeaacIcs *d_ics,
                                       const HeaacSbrFrame *d_sbr,
                                       const HeaacSbrHeader *d_hdr, size_t n_hdr,
                                       const HeaacPsFrame *d_ps,
                                       const float *d_state_in, float *d_state_out,
                                       void *d_pcm, int pcm_format,
                                       size_t n_streams, size_t frames_per_stream, void *stream)
{
    return heaac_he_decode_streams_ex(dev, cfg, flags, d_coeffs, d_ics, d_sbr, d_hdr, n_hdr, d_ps, d_state_in, d_state_out,
                                      d_pcm, pcm_format, n_streams, frames_per_stream, NULL, stream);
}

extern "C" int heaac_he_decode_streams_ex(HeaacDevice *dev, int cfg, int flags,
                                          const float *d_coeffs, const HeaacIcs *d_ics,
                                          const HeaacSbrFrame *d_sbr,
                                          const HeaacSbrHeader *d_hdr, size_t n_hdr,
                                          const HeaacPsFrame *d_ps,
                                          const float *d_state_in, float *d_state_out,
                                          void *d_pcm, int pcm_format,
                                          size_t n_streams, size_t frames_per_stream,
                                          const uint8_t *d_hold, void *stream)
{
    if (!dev || !he_cfg_ok(cfg) || !pcm_format_ok(pcm_format) || (flags & ~HEAAC_HE_DOWNSAMPLED) ||
        frames_per_stream == 0 || frames_per_stream > heaac_device_max_frames_per_stream(dev))
        return HEAAC_ERR_ARG;
    if (n_streams == 0)
        return HEAAC_OK;
    if (!d_coeffs || !d_ics || !d_sbr || !d_hdr || !n_hdr || !d_state_in || !d_state_out || !d_pcm ||
        (cfg == HEAAC_CFG_HEV2 && !d_ps))
        return HEAAC_ERR_ARG;
    return he_walk(dev, cfg, flags, d_coeffs, d_ics, d_sbr, d_hdr, n_hdr, d_ps, d_state_in, d_state_out, d_pcm,
                   pcm_format, n_streams, frames_per_stream, d_hold, (hipStream_t)stream);
}

extern "C" int heaac_qmf_analysis_batch(HeaacDevice *dev, const float *d_in,
                                        const float *d_xhist_in, float *d_xhist_out,
                                        float *d_W, float scale, size_t n, void *stream)
{
    if (!dev) return HEAAC_ERR_ARG;
    if (n == 0) return HEAAC_OK;
    if (!d_in || !d_xhist_in || !d_xhist_out || !d_W) return HEAAC_ERR_ARG;
    return heaac_launch_qmf_analysis(dev->d_tab, d_in, d_xhist_in, d_xhist_out, d_W, scale, n,
                                     (hipStream_t)stream);
}

extern "C" int heaac_qmf_synthesis_batch(HeaacDevice *dev, const float *d_X,
                                         const float *d_v_in, float *d_v_out,
                                         float *d_out, float scale, float bias,
                                         size_t n, void *stream)
{
    if (!dev) return HEAAC_ERR_ARG;
    if (n == 0) return HEAAC_OK;
    if (!d_X || !d_v_in || !d_v_out || !d_out) return HEAAC_ERR_ARG;
    return heaac_launch_qmf_synthesis(dev->d_tab, d_X, d_v_in, d_v_out, d_out, scale, bias, n,
                                      (hipStream_t)stream);
}

extern "C" int heaac_qmf_synthesis_ds_batch(HeaacDevice *dev, const float *d_X,
                                            const float *d_v_in, float *d_v_out,
                                            float *d_out, float scale, float bias,
                                            size_t n, void *stream)
{
    if (!dev) return HEAAC_ERR_ARG;
    if (n == 0) return HEAAC_OK;
    if (!d_X || !d_v_in || !d_v_out || !d_out) return HEAAC_ERR_ARG;
    return heaac_launch_qmf_synthesis_ds(dev->d_tab, d_X, d_v_in, d_v_out, d_out, scale, bias, n,
                                         (hipStream_t)stream);
}

extern "C" int heaac_couple_after_imdct_batch(HeaacDevice *dev, int channels, float *d_pcm, const float *d_cce,
                                              const HeaacCoupling *d_coupling, int16_t *d_s16,
                                              size_t n, void *stream)
{
    if (!dev || (channels != 1 && channels != 2)) return HEAAC_ERR_ARG;
    if (n == 0) return HEAAC_OK;
    if (!d_pcm || !d_cce || !d_coupling || n > 0x7fffffffu) return HEAAC_ERR_ARG;
    return heaac_launch_couple(channels, d_pcm, d_cce, d_coupling, d_s16, n, (hipStream_t)stream);
}

extern "C" int heaac_pcm_interleave_batch(HeaacDevice *dev, int channels, const HeaacPlaneRef *planes, int len,
                                          int pcm_format, int16_t *d_out, size_t n, void *stream)
{
    if (!dev || channels < 1 || channels > HEAAC_MAX_PCM_PLANES || len <= 0 || (len & 3) ||
        (pcm_format != HEAAC_PCM_S16_INTERLEAVED && pcm_format != HEAAC_PCM_S16_INTERLEAVED_SSE2))
        return HEAAC_ERR_ARG;
    if (n == 0) return HEAAC_OK;
    if (!planes || !d_out) return HEAAC_ERR_ARG;
    for (int c = 0; c < channels; c++)
        if (!planes[c].d_base || ((uintptr_t)planes[c].d_base & 15) || (planes[c].frame_stride & 3)) return HEAAC_ERR_ARG;
    return heaac_launch_interleave(channels, planes, len, pcm_format, d_out, n, (hipStream_t)stream);
}

// include/heaac_debug.h: device pointers of workspace set 0
extern "C" int heaac_debug_workspace(HeaacDevice *dev, float **d_W, float **d_X, size_t *chunk)
{
    if (!dev) return HEAAC_ERR_ARG;
    if (d_W) *d_W = (float *)dev->d_work;
    if (d_X) *d_X = (float *)dev->d_work + dev->chunk * WS_W_FLOATS;      /* set 0 */
    if (chunk) *chunk = dev->chunk;
    return HEAAC_OK;
}

extern "C" int heaac_debug_xbands(HeaacDevice *dev, unsigned char *host_out, size_t n_frames)
{
    // chunk c of a call writes its records at 2 (c mod sets) chunk: for the first `sets` chunks that is 2 f0, so the
    // records of up to sets x chunk frames lie in frame order
    if (!dev || !host_out || n_frames > (size_t)(dev->sets > 0 ? dev->sets : 1) * dev->chunk) return HEAAC_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return HEAAC_ERR_HIP;
    return hipMemcpy(host_out, dev->d_aux + HE_ZERO_BYTES, 2 * n_frames, hipMemcpyDeviceToHost) == hipSuccess
               ? HEAAC_OK : HEAAC_ERR_HIP;
}

// internal (host_common.h): the most frames per stream the HE streams calls take on this device -- whole streams go
// through one workspace set of `chunk` frames
size_t heaac_device_max_frames_per_stream(const HeaacDevice *dev) { return dev ? dev->chunk : 0; }

// internal: device table pointers for shim.hip
extern "C" const float *heaac_device_tables(HeaacDevice *dev, const uint16_t **rev)
{
    if (rev) *rev = dev->d_rev;
    return dev->d_tab;
}
