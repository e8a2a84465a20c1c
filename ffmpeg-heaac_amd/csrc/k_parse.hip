// k_parse.hip -- heaac_sbr_parse_device: the payload walk of sbr_core.h, one lane per unit.
//
// k_sbr_parse: 64 units per wave, one wave per block, the 3.4 KB of code-book nodes in LDS.  sbr_core.h is the one
// writing of the payload syntax: the host parser (sbr_parse.c) reads through the same sc_* functions and adds header
// registration, roll-backs and statuses; the device defers every unit that needs one of those (sc_walk).  The prep
// kernel of k_parse_streams.hip runs ahead of it (heaac_launch_parse_prep: the state rows copied in -> out, the records
// zeroed); the walk works on the out row and a lane that gives its unit up copies the row once more.
// heaac_debug_sbr_parse_core is the host form.
//
// The AAC walk of heaac_aac_parse_device stands in k_parse_streams.hip with every other caller of pc_walk.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "heaac_dsp.h"
#include "heaac_parse.h"
#include "heaac_debug.h"
#include "parse_core.h"
#include "sbr_core.h"
#include "parse_streams.h"
#include "kernels.h"

// One unit on either side: the AAC status gate, the walk on the out row (which holds the in row), the row copied again
// where the unit is given up.  Returns 0 or the SC_WHY_* reason.
static __host__ __device__ inline int sbr_unit(const HeaacAacConfig *cfg, const HeaacSbrParseTables *t, const HeaacSbrStream *st_in,
                                               HeaacSbrStream *st_out, const uint8_t *au, const uint32_t *au_offset, size_t i,
                                               const HeaacAacFrameInfo *info, const int32_t *aac_status, const HeaacSbrHeader *hdr,
                                               uint32_t n_hdr, HeaacSbrFrame *sbr, HeaacPsFrame *ps)
{
    int r = SC_WHY_AAC;
    if (!aac_status || aac_status[i] == HEAAC_PARSE_OK) {
        const uint32_t lo = au_offset[i], hi = au_offset[i + 1];
        r = SC_WHY_REFUSED;
        if (hi > lo && hi - lo < PARSE_MAX_UNIT)
            r = sc_walk(cfg, t, st_out + i, au + lo, (int)(hi - lo), info + i, hdr, n_hdr, sbr + i, ps ? ps + i : NULL);
    }
    if (r) {
        const uint32_t *src = (const uint32_t *)(st_in + i);
        uint32_t *dst = (uint32_t *)(st_out + i);
        for (unsigned k = 0; k < sizeof(HeaacSbrStream) / 4; k++) dst[k] = src[k];
    }
    return r;
}

__global__ __launch_bounds__(PARSE_BLOCK) void k_sbr_parse(HeaacAacConfig cfg, const HeaacSbrParseTables *t, const HeaacSbrStream *st_in,
                                                           HeaacSbrStream *st_out, const uint8_t *au, const uint32_t *au_offset,
                                                           const HeaacAacFrameInfo *info, const int32_t *aac_status,
                                                           unsigned long long n, const HeaacSbrHeader *hdr, uint32_t n_hdr,
                                                           HeaacSbrFrame *sbr, HeaacPsFrame *ps, int32_t *status)
{
    __shared__ uint4 s_tab[sizeof(HeaacSbrParseTables) / 16];
    const uint4 *src = (const uint4 *)t;
    for (int k = threadIdx.x; k < (int)(sizeof(HeaacSbrParseTables) / 16); k += PARSE_BLOCK) s_tab[k] = src[k];
    __syncthreads();
    const unsigned long long i = (unsigned long long)blockIdx.x * PARSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int r = sbr_unit(&cfg, (const HeaacSbrParseTables *)s_tab, st_in, st_out, au, au_offset, (size_t)i, info, aac_status, hdr,
                           n_hdr, sbr, ps);
    status[i] = r ? HEAAC_PARSE_DEFERRED : HEAAC_PARSE_OK;
}

int heaac_launch_sbr_parse(const HeaacSbrParseTables *d_tab, const HeaacAacConfig *cfg, const HeaacSbrStream *d_sst_in,
                           HeaacSbrStream *d_sst_out, const uint8_t *d_au, const uint32_t *d_au_offset,
                           const HeaacAacFrameInfo *d_info, const int32_t *d_aac_status, size_t n, const HeaacSbrHeader *d_hdr,
                           size_t n_hdr, HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps, int32_t *d_status, hipStream_t s)
{
    if (n > PARSE_GRID_MAX || n > SIZE_MAX / sizeof(HeaacSbrStream)) return HEAAC_ERR_ARG;
    const unsigned long long blocks = ((unsigned long long)n + PARSE_BLOCK - 1) / PARSE_BLOCK;
    heaac_launch_parse_prep(NULL, 0, d_sst_in, d_sst_out, (unsigned long long)n * (sizeof(HeaacSbrStream) / 4), d_sbr,
                            (unsigned long long)n * (sizeof(HeaacSbrFrame) / 4), d_ps,
                            d_ps ? (unsigned long long)n * (sizeof(HeaacPsFrame) / 4) : 0ull, s);
    hipLaunchKernelGGL(k_sbr_parse, dim3((unsigned)blocks), dim3(PARSE_BLOCK), 0, s, *cfg, d_tab, d_sst_in, d_sst_out, d_au, d_au_offset,
                       d_info, d_aac_status, (unsigned long long)n, d_hdr, (uint32_t)(n_hdr > 0xffffffffull ? 0xffffffffull : n_hdr),
                       d_sbr, d_ps, d_status);
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

// what both forms refuse before they look at a unit (n > 0)
int heaac_sbr_parse_args_ok(const HeaacAacConfig *cfg, const void *sst_in, const void *sst_out, const void *au, const void *au_offset,
                            const void *info, size_t n, const void *hdr, size_t n_hdr, const void *sbr, const void *ps,
                            const void *status)
{
    if (!cfg || !sst_in || !sst_out || !au || !au_offset || !info || !hdr || !sbr || !status || n_hdr == 0) return 0;
    if (cfg->ps != 0 && cfg->chan_config == 1 && !ps) return 0;
    if (n > SIZE_MAX / sizeof(HeaacSbrStream)) return 0;
    const uintptr_t a = (uintptr_t)sst_in, b = (uintptr_t)sst_out, len = n * sizeof(HeaacSbrStream);
    if (a < b + len && b < a + len) return 0;          // the state arrays overlap
    return !((a | b | (uintptr_t)au_offset | (uintptr_t)info | (uintptr_t)hdr | (uintptr_t)sbr | (uintptr_t)ps | (uintptr_t)status) & 3);
}

extern "C" int heaac_debug_sbr_parse_core(const HeaacAacConfig *cfg, const HeaacSbrStream *sst_in, HeaacSbrStream *sst_out,
                                          const uint8_t *au, const uint32_t *au_offset, const HeaacAacFrameInfo *info,
                                          const int32_t *aac_status, size_t n, const HeaacSbrHeader *hdr, size_t n_hdr,
                                          HeaacSbrFrame *sbr, HeaacPsFrame *ps, int32_t *status, int32_t *why)
{
    if (!cfg) return HEAAC_ERR_ARG;
    if (n == 0) return HEAAC_OK;
    if (!heaac_sbr_parse_args_ok(cfg, sst_in, sst_out, au, au_offset, info, n, hdr, n_hdr, sbr, ps, status)) return HEAAC_ERR_ARG;
    const HeaacSbrParseTables *t = heaac_sbr_parse_tables();
    if (!t) return HEAAC_ERR_ARG;
    memcpy(sst_out, sst_in, n * sizeof(*sst_out));
    memset(sbr, 0, n * sizeof(*sbr));
    if (ps) memset(ps, 0, n * sizeof(*ps));
    for (size_t i = 0; i < n; i++) {
        const int r = sbr_unit(cfg, t, sst_in, sst_out, au, au_offset, i, info, aac_status, hdr,
                               (uint32_t)(n_hdr > 0xffffffffull ? 0xffffffffull : n_hdr), sbr, ps);
        status[i] = r ? HEAAC_PARSE_DEFERRED : HEAAC_PARSE_OK;
        if (why) why[i] = r;
    }
    return HEAAC_OK;
}
