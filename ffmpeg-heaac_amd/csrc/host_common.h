// host_common.h -- internal: the host-side decisions that the pipelines (pipeline.hip, pipeline_layout.hip), the
// codec contexts (shim.hip, codec_layout.hip), the layout walk they share (layout_common.hip) and the C ABI (capi.hip)
// share.  Not part of include/*.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "heaac_dsp.h"
#include "heaac_parse.h"

#define HIP_OK(x) do { if ((x) != hipSuccess) return HEAAC_ERR_HIP; } while (0)

static inline int pinned(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess; }
static inline int devmem(void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess; }

// ---- what an object owns ----
// Every block an object allocates is recorded with its owner, and destroy releases the list: no free list to keep in
// step with create, and a half-built object is released the same way.  HOST blocks are zeroed (calloc).
struct HeaacMem;
enum { HEAAC_MEM_HOST, HEAAC_MEM_PINNED, HEAAC_MEM_DEVICE };
int heaac_mem(HeaacMem **owner, int kind, void **p, size_t bytes);          // 1: *p allocated and recorded
void heaac_mem_release(HeaacMem **owner);
template <class T> static inline int heaac_host(HeaacMem **o, T **p, size_t bytes) { return heaac_mem(o, HEAAC_MEM_HOST, (void **)p, bytes); }
template <class T> static inline int heaac_dev(HeaacMem **o, T **p, size_t bytes) { return heaac_mem(o, HEAAC_MEM_DEVICE, (void **)p, bytes); }
// a buffer the host fills and the device reads, or the other way round: pinned host memory and its device twin
template <class T> static inline int heaac_pair(HeaacMem **o, T **h, T **d, size_t bytes)
{
    return heaac_mem(o, HEAAC_MEM_PINNED, (void **)h, bytes) && heaac_mem(o, HEAAC_MEM_DEVICE, (void **)d, bytes);
}

// ---- configuration -> shape ----
struct HeaacCfgShape {
    int ncore, nout;              // core channels, output channels; ncore = 0: not a configuration
    int he;                       // SBR behind the core (2048 samples per frame unless downsampled)
    size_t words;                 // state words per stream
    // where the parts of a stream's state record begin (the saved overlap is at 0): [ncore] SBR, [nout] synthesis, PS
    int off_sbr, off_syn, off_ps;
};
HeaacCfgShape heaac_cfg_shape(int cfg);
// the largest state record of the configurations: what a context allocates before its stream has said which it is
#define HEAAC_STATE_WORDS_MAX (HEAAC_STATE_WORDS_HEV2 > HEAAC_STATE_WORDS_HEV1 ? HEAAC_STATE_WORDS_HEV2 : HEAAC_STATE_WORDS_HEV1)

// ---- parser worker pool ----
// Persistent threads that run fn(ctx, slice, phase) for the slices 0 .. threads-1 of a job: slice w owns the streams
// [n w / W, n (w + 1) / W) and their parser state, W = heaac_pool_threads().
struct HeaacPool;
typedef void (*HeaacSliceFn)(void *ctx, int slice, int phase);
// `threads` >= 1, already clamped by the caller.  Where pthread_create fails part-way the pool runs with the threads
// it got: size per-slice storage and partition by heaac_pool_threads().  NULL: out of memory.
HeaacPool *heaac_pool_create(int threads, HeaacSliceFn fn, void *ctx);
int heaac_pool_threads(const HeaacPool *pool);
// every slice of one phase: slice 0 on the calling thread, the others on the workers; returns when all are done.
// (What the caller wrote before the call is visible to the workers.)
void heaac_pool_run(HeaacPool *pool, int phase);
void heaac_pool_destroy(HeaacPool *pool);
// Parser threads when the caller does not say.  The two pipelines differ, and stay so: heaac_pipeline takes the CPUs
// the process may actually use (the cgroup CPU quota), heaac_layout_pipeline the online count, at most 32.
int heaac_threads_by_cpu_quota(void);
int heaac_threads_online_max32(void);

// ---- rows of the streams whose unit failed (the layout pipeline, pipeline_layout.hip: its spectral tools call takes
// coupling elements and has no streams form with hold masks, so it parks the failed streams' rows around its calls) ----
// One block of `block` threads per (stream, parking row) pair of d_list, rows of row_words 32-bit words:
//   mode 0: park[row] = rows[stream];  1: rows[stream] = park[row];  2: rows[stream] = 0 (park may be NULL)
void heaac_rows(hipStream_t s, const unsigned *d_list, unsigned pairs, unsigned block, void *rows, void *park,
                size_t row_words, int mode);
// failed[n] -> two lists of (stream, parking row) in h_list, uploaded to d_list on s: at [0, 2 n) every failed stream
// (its DSP state, its PCM row), at [2 n, 4 n) those of them whose generator and predictors stay put as well
// (failed == 1; 2: the tools' side of the stream moves on).  A stream's parking row is its place in the first list.
int heaac_failed_lists(hipStream_t s, const unsigned char *failed, size_t n, unsigned *h_list, unsigned *d_list,
                       unsigned *n_all, unsigned *n_full);
// A parking area of `have` rows that must hold `needed`: *rows = have where it does; else s is drained (nothing of the
// old area is in flight then, the caller frees it) and *rows = first, doubled until it holds them, at most n.
int heaac_park_grow(hipStream_t s, size_t needed, size_t have, size_t first, size_t n, size_t *rows);

// ---- the kernels of a device-parse tick (k_fix.hip; pipeline.hip) ----
// The five record arrays of a tick, in the order coefficients, HeaacIcs, tools, SBR, PS: where the tick's rows and the
// staged rows begin and the 32-bit words of one unit's row (0: the configuration has no such array).
#define HEAAC_FIX_ARRAYS 5
struct HeaacFixRows {
    uint32_t *dst[HEAAC_FIX_ARRAYS];
    const uint32_t *src[HEAAC_FIX_ARRAYS];
    uint32_t words[HEAAC_FIX_ARRAYS];
};
// Behind the walk: host_status[i] (the device's view of mapped host memory; NULL: not wanted) = d_status[i], with
// HEAAC_PARSE_OK -> HEAAC_PARSE_NO_SBR where an HE unit had no payload (sbr_off: the configuration has no SBR at all);
// d_hold_tools[0 .. nf) = 0.
__attribute__((visibility("hidden"))) int heaac_launch_parse_status(hipStream_t s, const int32_t *d_status,
                                                                    const HeaacAacFrameInfo *d_info, int he, int sbr_off,
                                                                    int32_t *host_status, uint8_t *d_hold_tools, size_t nf);
// State rows d_list[j] of d_ast (and of d_sst unless NULL) -> row j of the compact buffers (device memory, or the
// device's view of mapped host memory), j < m.
__attribute__((visibility("hidden"))) int heaac_launch_fix_gather(hipStream_t s, const uint32_t *d_list, size_t m,
                                                                  const HeaacAacStream *d_ast, void *d_g_ast,
                                                                  const HeaacSbrStream *d_sst, void *d_g_sst);
// Staged unit u < units: its rows to row d_dest[u] of the tick's arrays, d_staged_hold[u] and [units + u] to d_hold
// [d_dest[u]] and [nf + d_dest[u]]; the compact state rows back to the rows d_list names.
__attribute__((visibility("hidden"))) int heaac_launch_fix_scatter(hipStream_t s, const HeaacFixRows *rows, const uint32_t *d_dest,
                                                                   size_t units, const uint8_t *d_staged_hold, uint8_t *d_hold,
                                                                   size_t nf, const uint32_t *d_list, size_t m, const void *d_g_ast,
                                                                   HeaacAacStream *d_ast, const void *d_g_sst, HeaacSbrStream *d_sst);

// ---- the device (capi.hip) ----
// The most frames per stream heaac_he_decode_streams(_ex) takes on this device: a stream's frames go through one
// workspace set.  The call's own argument check and heaac_pipeline_create_streams both ask here.
size_t heaac_device_max_frames_per_stream(const HeaacDevice *dev);

// ---- per-stream device state at create ----
// ac->random_state of n streams (aacdec.c:558); reset_predict_state (aacdec.c:507-515) for `count` predictors
int heaac_seed_generators(int32_t *d_rng, size_t n);                         // 1: done
int heaac_reset_predictors(HeaacPredictorState *d_pred, size_t count);      // 1: done

// ---- SBR header records ----
// What the table has gained since *uploaded -> d_hdr (the table's storage never moves).  With a host `mirror` (the
// copy heaac_validate_frame reads in the codec contexts) it is brought up to date too and the upload is synchronous;
// without one the upload rides on s.
int heaac_upload_headers(const HeaacSbrHeaderTable *tab, size_t *uploaded, HeaacSbrHeader *d_hdr, HeaacSbrHeader *mirror,
                         hipStream_t s);
