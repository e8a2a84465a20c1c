// host_common.hip -- host_common.h: what an object owns, the worker pool, the parking of failed streams' rows (the
// layout pipeline's), per-stream device seeding, the SBR header upload and the configuration's shape, once for the
// pipelines, the codec contexts and the C ABI.
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "host_common.h"

HeaacCfgShape heaac_cfg_shape(int cfg)
{
    HeaacCfgShape c = {};
    switch (cfg) {
    case HEAAC_CFG_LC_MONO:   c = { 1, 1, 0, HEAAC_STATE_WORDS_LC_MONO }; break;
    case HEAAC_CFG_LC_STEREO: c = { 2, 2, 0, HEAAC_STATE_WORDS_LC_STEREO }; break;
    case HEAAC_CFG_HEV1:      c = { 2, 2, 1, HEAAC_STATE_WORDS_HEV1 }; break;
    case HEAAC_CFG_HEV1_MONO: c = { 1, 1, 1, HEAAC_STATE_WORDS_HEV1_MONO }; break;
    case HEAAC_CFG_HEV2:      c = { 1, 2, 1, HEAAC_STATE_WORDS_HEV2 }; break;
    default: return c;
    }
    // the record of include/heaac_dsp.h: [ncore] saved overlap | [ncore] SBR | [nout] synthesis | PS (HE-AACv2)
    c.off_sbr = c.ncore * HEAAC_ST_SAVED;
    c.off_syn = c.off_sbr + c.he * c.ncore * HEAAC_ST_SBR;
    c.off_ps = c.off_syn + c.he * c.nout * HEAAC_ST_SYNTH;
    return c;
}

// ---------------------------------------------------------------------------
// what an object owns
// ---------------------------------------------------------------------------
struct HeaacMem { HeaacMem *next; void *p; int kind; };

int heaac_mem(HeaacMem **owner, int kind, void **p, size_t bytes)
{
    HeaacMem *m = (HeaacMem *)malloc(sizeof(*m));
    if (!m) return 0;
    *p = NULL;
    const int ok = kind == HEAAC_MEM_HOST ? (*p = calloc(1, bytes)) != NULL : kind == HEAAC_MEM_PINNED ? pinned(p, bytes) : devmem(p, bytes);
    if (!ok) { *p = NULL; free(m); return 0; }
    m->next = *owner; m->p = *p; m->kind = kind;
    *owner = m;
    return 1;
}

void heaac_mem_release(HeaacMem **owner)
{
    while (*owner) {
        HeaacMem *m = *owner;
        *owner = m->next;
        if (m->kind == HEAAC_MEM_HOST) free(m->p);
        else if (m->kind == HEAAC_MEM_PINNED) (void)hipHostFree(m->p);
        else (void)hipFree(m->p);
        free(m);
    }
}

// ---------------------------------------------------------------------------
// worker pool
// ---------------------------------------------------------------------------
struct HeaacPool {
    HeaacSliceFn fn; void *ctx;
    int threads, phase;
    pthread_t *tid;
    pthread_mutex_t mu;
    pthread_cond_t cv_go, cv_done;
    unsigned long generation;
    int pending, quit;
};

struct PoolWorkerArg { HeaacPool *pool; int w; };

static void *pool_worker(void *arg)
{
    PoolWorkerArg *a = (PoolWorkerArg *)arg;
    HeaacPool *p = a->pool;
    const int w = a->w;
    free(a);
    unsigned long seen = 0;
    pthread_mutex_lock(&p->mu);
    for (;;) {
        while (p->generation == seen && !p->quit) pthread_cond_wait(&p->cv_go, &p->mu);
        if (p->quit) break;
        seen = p->generation;
        const int phase = p->phase;
        pthread_mutex_unlock(&p->mu);
        p->fn(p->ctx, w, phase);
        pthread_mutex_lock(&p->mu);
        if (--p->pending == 0) pthread_cond_signal(&p->cv_done);
    }
    pthread_mutex_unlock(&p->mu);
    return NULL;
}

HeaacPool *heaac_pool_create(int threads, HeaacSliceFn fn, void *ctx)
{
    HeaacPool *p = (HeaacPool *)calloc(1, sizeof(*p));
    if (!p) return NULL;
    p->fn = fn; p->ctx = ctx;
    p->threads = threads;
    pthread_mutex_init(&p->mu, NULL);
    pthread_cond_init(&p->cv_go, NULL);
    pthread_cond_init(&p->cv_done, NULL);
    p->tid = (pthread_t *)calloc(threads, sizeof(pthread_t));
    bool ok = p->tid != NULL;
    for (int t = 1; t < threads && ok; t++) {          // slice 0 runs on the submitting thread
        PoolWorkerArg *a = (PoolWorkerArg *)malloc(sizeof(*a));
        if (!a) { ok = false; break; }
        a->pool = p; a->w = t;
        if (pthread_create(&p->tid[t], NULL, pool_worker, a) != 0) { free(a); p->tid[t] = 0; p->threads = t; break; }
    }
    if (!ok) { heaac_pool_destroy(p); return NULL; }
    return p;
}

int heaac_pool_threads(const HeaacPool *pool) { return pool->threads; }

void heaac_pool_run(HeaacPool *p, int phase)
{
    pthread_mutex_lock(&p->mu);
    p->phase = phase;
    p->pending = p->threads - 1;
    p->generation++;
    pthread_cond_broadcast(&p->cv_go);
    pthread_mutex_unlock(&p->mu);
    p->fn(p->ctx, 0, phase);
    pthread_mutex_lock(&p->mu);
    while (p->pending > 0) pthread_cond_wait(&p->cv_done, &p->mu);
    pthread_mutex_unlock(&p->mu);
}

void heaac_pool_destroy(HeaacPool *p)
{
    if (!p) return;
    pthread_mutex_lock(&p->mu);
    p->quit = 1;
    pthread_cond_broadcast(&p->cv_go);
    pthread_mutex_unlock(&p->mu);
    for (int t = 1; p->tid && t < p->threads; t++) if (p->tid[t]) pthread_join(p->tid[t], NULL);
    free(p->tid);
    pthread_cond_destroy(&p->cv_go); pthread_cond_destroy(&p->cv_done); pthread_mutex_destroy(&p->mu);
    free(p);
}

// Inside a container the CPU bandwidth quota (cgroup v2 cpu.max) can be far below the online count; threads beyond
// about twice the quota only get throttled (measured on the GPU box: 256 online, quota 16: 32 threads parse a tick
// in 6 ms, 256 in 18 ms once the copy engines' helper threads compete).
int heaac_threads_by_cpu_quota(void)
{
    long online = sysconf(_SC_NPROCESSORS_ONLN);
    if (online < 1) online = 1;
    FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (f) {
        long long quota = 0, period = 0;
        if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) {
            const long cap = (long)((2 * quota + period - 1) / period);
            if (cap >= 1 && cap < online) online = cap;
        }
        fclose(f);
    }
    return (int)online;
}

int heaac_threads_online_max32(void)
{
    const long online = sysconf(_SC_NPROCESSORS_ONLN);
    return online < 1 ? 1 : online > 32 ? 32 : (int)online;
}

// ---------------------------------------------------------------------------
// rows of the failed streams
// ---------------------------------------------------------------------------
// Rows of the listed streams to the parking area and back (or zeroed): one block per (stream, parking row) pair.  A
// tick of the layout pipeline with thousands of damaged units costs a handful of launches, not six copies per stream
// (tools/layout_rate.py --damaged).
__global__ void k_rows(const unsigned *__restrict__ list, unsigned *rows, unsigned *park, unsigned long long row_words, int mode)
{
    const unsigned stream = list[2 * blockIdx.x], slot = list[2 * blockIdx.x + 1];
    unsigned *r = rows + stream * row_words;
    unsigned *q = park ? park + slot * row_words : nullptr;
    for (unsigned long long w = threadIdx.x; w < row_words; w += blockDim.x) {
        if (mode == 0) q[w] = r[w];
        else if (mode == 1) r[w] = q[w];
        else r[w] = 0u;
    }
}

void heaac_rows(hipStream_t s, const unsigned *d_list, unsigned pairs, unsigned block, void *rows, void *park,
                size_t row_words, int mode)
{
    hipLaunchKernelGGL(k_rows, dim3(pairs), dim3(block), 0, s, d_list, (unsigned *)rows, (unsigned *)park,
                       (unsigned long long)row_words, mode);
}

int heaac_failed_lists(hipStream_t s, const unsigned char *failed, size_t n, unsigned *h_list, unsigned *d_list,
                       unsigned *n_all_out, unsigned *n_full_out)
{
    unsigned n_all = 0, n_full = 0;
    unsigned *list_all = h_list, *list_full = h_list + 2 * n;
    for (size_t i = 0; i < n; i++) {
        if (!failed[i]) continue;
        if (failed[i] == 1) { list_full[2 * n_full] = (unsigned)i; list_full[2 * n_full + 1] = n_all; n_full++; }
        list_all[2 * n_all] = (unsigned)i; list_all[2 * n_all + 1] = n_all; n_all++;
    }
    *n_all_out = n_all; *n_full_out = n_full;
    if (n_all) HIP_OK(hipMemcpyAsync(d_list, list_all, 2 * n_all * sizeof(unsigned), hipMemcpyHostToDevice, s));
    if (n_full)
        HIP_OK(hipMemcpyAsync(d_list + 2 * n, list_full, 2 * n_full * sizeof(unsigned), hipMemcpyHostToDevice, s));
    return HEAAC_OK;
}

int heaac_park_grow(hipStream_t s, size_t needed, size_t have, size_t first, size_t n, size_t *rows)
{
    *rows = have;
    if (needed <= have) return HEAAC_OK;
    HIP_OK(hipStreamSynchronize(s));
    size_t r = first;
    while (r < needed) r *= 2;
    *rows = r > n ? n : r;
    return HEAAC_OK;
}

// ---------------------------------------------------------------------------
// per-stream device state at create, header records
// ---------------------------------------------------------------------------
int heaac_seed_generators(int32_t *d_rng, size_t n)
{
    int32_t *seed = (int32_t *)malloc(n * 4);
    if (!seed) return 0;
    for (size_t i = 0; i < n; i++) seed[i] = 0x1f2e3d4c;
    const int ok = hipMemcpy(d_rng, seed, n * 4, hipMemcpyHostToDevice) == hipSuccess;
    free(seed);
    return ok;
}

int heaac_reset_predictors(HeaacPredictorState *d_pred, size_t count)
{
    HeaacPredictorState *ps = (HeaacPredictorState *)calloc(count, sizeof(*ps));
    if (!ps) return 0;
    for (size_t i = 0; i < count; i++) ps[i].var0 = ps[i].var1 = 1.0f;
    const int ok = hipMemcpy(d_pred, ps, count * sizeof(*ps), hipMemcpyHostToDevice) == hipSuccess;
    free(ps);
    return ok;
}

int heaac_upload_headers(const HeaacSbrHeaderTable *tab, size_t *uploaded, HeaacSbrHeader *d_hdr, HeaacSbrHeader *mirror,
                         hipStream_t s)
{
    const size_t have = heaac_sbr_table_count(tab), from = *uploaded;
    if (have <= from) return HEAAC_OK;
    const size_t bytes = (have - from) * sizeof(HeaacSbrHeader);
    if (mirror) {
        memcpy(mirror + from, heaac_sbr_table_data(tab) + from, bytes);
        HIP_OK(hipMemcpy(d_hdr + from, mirror + from, bytes, hipMemcpyHostToDevice));
    } else {
        HIP_OK(hipMemcpyAsync(d_hdr + from, heaac_sbr_table_data(tab) + from, bytes, hipMemcpyHostToDevice, s));
    }
    *uploaded = have;
    return HEAAC_OK;
}
