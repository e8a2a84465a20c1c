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
// The same walk is instantiated for the host as heaac_debug_aac_parse_core (include/heaac_debug.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "heaac_dsp.h"
#include "heaac_parse.h"
#include "heaac_debug.h"
#include "parse_core.h"
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
