// k_parse.hip -- heaac_aac_parse_device: the access-unit walk of parse_core.h, one lane per unit.
//
// 64 units per wave, one wave per block (a tick of 32 768 streams is 512 waves: two per CU).  The twelve ten-bit
// prefix tables (48 KB) are copied to LDS at the head of the block, the tree nodes behind them, the dequantisation
// tables and the band tables stay in global memory (read-only, shared by every lane: they live in L2).  Per-band
// arrays are written straight into the unit's HeaacToolsFrame and read back from there, so the walk keeps no
// runtime-indexed private array; a quad codeword leaves as one 16-byte store, a pair as one 8-byte store.  The
// records are zeroed ahead of the walk by a fill kernel of the same call (every lane of the grid, 16-byte stores): a
// kernel and not hipMemsetAsync (its graph node left the records unzeroed on replay with ROCm 7.0's runtime).
//
// The same walk is instantiated for the host as heaac_debug_aac_parse_core (include/heaac_debug.h).  parse_core.h is the
// one writing of the element syntax: the host parser (aac_parse.c) reads through the same pc_* functions with a PcHost
// record for its statuses, refusal progress and pulse data; the walk passes NULL and defers every such unit.
//
// heaac_sbr_parse_device: the payload walk of sbr_core.h in the same layout (k_sbr_parse, one lane per unit, the 3.4 KB
// of code-book nodes in LDS).  sbr_core.h is the one writing of the payload syntax: the host parser (sbr_parse.c) reads
// through the same sc_* functions and adds header registration, roll-backs and statuses; the device defers every unit
// that needs one of those (sc_walk).  A kernel ahead of it (k_sbr_prep, every lane of the grid, coalesced words) copies
// the state rows in -> out and zeroes the records; the walk works on the out row and a lane that gives its unit up
// copies the row once more.  heaac_debug_sbr_parse_core is the host form.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "heaac_dsp.h"
#include "heaac_parse.h"
#include "heaac_debug.h"
#include "parse_core.h"
#include "sbr_core.h"
#include "kernels.h"

#define PARSE_BLOCK 64
#define PARSE_MAX_UNIT (1u << 27)      // bytes: the walk counts bits in an int

__global__ __launch_bounds__(PARSE_BLOCK) void k_aac_parse(HeaacAacConfig cfg, const HeaacParseTables *t, HeaacAacStream *st,
                                                           const uint8_t *au, const uint32_t *au_offset,
                                                           unsigned long long n, int coeff_channels, float *coeffs,
                                                           HeaacIcs *ics, HeaacToolsFrame *tools, HeaacAacFrameInfo *info,
                                                           int32_t *status)
{
    __shared__ uint4 s_lut[HEAAC_PT_BOOKS * HEAAC_PT_LUT / 4];
    const uint4 *src = (const uint4 *)&t->lut[0][0];
    for (int k = threadIdx.x; k < HEAAC_PT_BOOKS * HEAAC_PT_LUT / 4; k += PARSE_BLOCK) s_lut[k] = src[k];
    __syncthreads();
    const unsigned long long i = (unsigned long long)blockIdx.x * PARSE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t lo = au_offset[i], hi = au_offset[i + 1];
    int r = PC_WHY_REFUSED;
    if (hi > lo && hi - lo < PARSE_MAX_UNIT)
        r = pc_walk(&cfg, t, (const uint32_t *)s_lut, st + i, au + lo, (int)(hi - lo), coeff_channels,
                    coeffs + i * (size_t)coeff_channels * 1024, ics + i * (size_t)coeff_channels, tools + i, info + i);
    status[i] = r ? HEAAC_PARSE_DEFERRED : HEAAC_PARSE_OK;
}

// p[0 .. words) = 0; p is 4-byte aligned (HeaacToolsFrame holds floats)
__global__ __launch_bounds__(256) void k_parse_zero(uint32_t *p, unsigned long long words)
{
    unsigned long long head = ((16 - ((uintptr_t)p & 15)) & 15) >> 2;
    if (head > words) head = words;
    const unsigned long long body = (words - head) >> 2, tail = (words - head) & 3;
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
    uint4 *q = (uint4 *)(p + head);
    if (gid < head) p[gid] = 0;
    for (unsigned long long k = gid; k < body; k += stride) q[k] = make_uint4(0, 0, 0, 0);
    if (gid < tail) p[head + body * 4 + gid] = 0;
}

int heaac_launch_aac_parse(const HeaacParseTables *d_tab, const HeaacAacConfig *cfg, HeaacAacStream *d_st,
                           const uint8_t *d_au, const uint32_t *d_au_offset, size_t n, int coeff_channels,
                           float *d_coeffs, HeaacIcs *d_ics, HeaacToolsFrame *d_tools, HeaacAacFrameInfo *d_info,
                           int32_t *d_status, hipStream_t s)
{
    const unsigned long long blocks = ((unsigned long long)n + PARSE_BLOCK - 1) / PARSE_BLOCK;
    if (blocks > 0x7fffffffull || n > SIZE_MAX / sizeof(HeaacToolsFrame)) return HEAAC_ERR_ARG;
    const unsigned long long words = (unsigned long long)n * (sizeof(HeaacToolsFrame) / 4);
    unsigned long long zb = (words / 4 + 255) / 256;
    zb = zb < 1 ? 1 : zb > 8192 ? 8192 : zb;
    hipLaunchKernelGGL(k_parse_zero, dim3((unsigned)zb), dim3(256), 0, s, (uint32_t *)d_tools, words);
    hipLaunchKernelGGL(k_aac_parse, dim3((unsigned)blocks), dim3(PARSE_BLOCK), 0, s, *cfg, d_tab, d_st, d_au, d_au_offset,
                       (unsigned long long)n, coeff_channels, d_coeffs, d_ics, d_tools, d_info, d_status);
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

// what both forms refuse before they look at a unit
int heaac_parse_args_ok(const HeaacAacConfig *cfg, int coeff_channels)
{
    return cfg && coeff_channels >= 1 && coeff_channels <= 2 && cfg->sampling_index >= 0 && cfg->sampling_index <= 12 &&
           (cfg->object_type == HEAAC_AOT_AAC_LC || cfg->object_type == HEAAC_AOT_AAC_MAIN);
}

extern "C" int heaac_debug_aac_parse_core(const HeaacAacConfig *cfg, HeaacAacStream *st, const uint8_t *au,
                                          const uint32_t *au_offset, size_t n, int coeff_channels, float *coeffs,
                                          HeaacIcs *ics, HeaacToolsFrame *tools, HeaacAacFrameInfo *info, int32_t *status,
                                          int32_t *why)
{
    if (!heaac_parse_args_ok(cfg, coeff_channels)) return HEAAC_ERR_ARG;
    if (n == 0) return HEAAC_OK;
    if (!st || !au || !au_offset || !coeffs || !ics || !tools || !info || !status) return HEAAC_ERR_ARG;
    const HeaacParseTables *t = heaac_parse_tables();
    if (!t) return HEAAC_ERR_ARG;
    for (size_t i = 0; i < n; i++) {
        const uint32_t lo = au_offset[i], hi = au_offset[i + 1];
        int r = PC_WHY_REFUSED;
        memset(tools + i, 0, sizeof(*tools));
        if (hi > lo && hi - lo < PARSE_MAX_UNIT)
            r = pc_walk(cfg, t, &t->lut[0][0], st + i, au + lo, (int)(hi - lo), coeff_channels,
                        coeffs + i * (size_t)coeff_channels * 1024, ics + i * (size_t)coeff_channels, tools + i, info + i);
        status[i] = r ? HEAAC_PARSE_DEFERRED : HEAAC_PARSE_OK;
        if (why) why[i] = r;
    }
    return HEAAC_OK;
}

// ---- the SBR / PS payload ----------------------------------------------------------------------------------------

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

// st_out[0 .. st_words) = st_in[..]; sbr[0 .. sbr_words) = 0; ps[0 .. ps_words) = 0 (all 4-byte aligned)
__global__ __launch_bounds__(256) void k_sbr_prep(const uint32_t *st_in, uint32_t *st_out, unsigned long long st_words, uint32_t *sbr,
                                                  unsigned long long sbr_words, uint32_t *ps, unsigned long long ps_words)
{
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
    for (unsigned long long k = gid; k < st_words; k += stride) st_out[k] = st_in[k];
    for (unsigned long long k = gid; k < sbr_words; k += stride) sbr[k] = 0;
    for (unsigned long long k = gid; k < ps_words; k += stride) ps[k] = 0;
}

int heaac_launch_sbr_parse(const HeaacSbrParseTables *d_tab, const HeaacAacConfig *cfg, const HeaacSbrStream *d_sst_in,
                           HeaacSbrStream *d_sst_out, const uint8_t *d_au, const uint32_t *d_au_offset,
                           const HeaacAacFrameInfo *d_info, const int32_t *d_aac_status, size_t n, const HeaacSbrHeader *d_hdr,
                           size_t n_hdr, HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps, int32_t *d_status, hipStream_t s)
{
    const unsigned long long blocks = ((unsigned long long)n + PARSE_BLOCK - 1) / PARSE_BLOCK;
    if (blocks > 0x7fffffffull || n > SIZE_MAX / sizeof(HeaacSbrStream)) return HEAAC_ERR_ARG;
    const unsigned long long st_words = (unsigned long long)n * (sizeof(HeaacSbrStream) / 4);
    unsigned long long pb = (st_words + 255) / 256;
    pb = pb > 8192 ? 8192 : pb;
    hipLaunchKernelGGL(k_sbr_prep, dim3((unsigned)pb), dim3(256), 0, s, (const uint32_t *)d_sst_in, (uint32_t *)d_sst_out, st_words,
                       (uint32_t *)d_sbr, (unsigned long long)n * (sizeof(HeaacSbrFrame) / 4), (uint32_t *)d_ps,
                       d_ps ? (unsigned long long)n * (sizeof(HeaacPsFrame) / 4) : 0ull);
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
