// k_parse_streams.hip -- the AAC walk of the device parsers and the kernel that prepares their records:
// heaac_aac_parse_device, heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams (the chain of
// parse_streams.h, one lane per STREAM), and the prep kernel of all of them and of heaac_sbr_parse_device (k_parse.hip).
//
// k_parse_streams<HE>: 64 streams per wave, one wave per block (a tick of 32 768 streams is 512 waves: two per CU); the
// lane loops over its T units, pc_walk and then (HE) sc_walk per unit, each from the state the unit before left, and
// stops at the first unit either gives up.  The twelve ten-bit prefix tables (48 KB) and, for HE, the 3 520 bytes of
// SBR / PS code-book nodes are copied to LDS at the head of the block; the tree nodes behind the prefix tables, the
// dequantisation tables and the band tables stay in global memory (read-only, shared by every lane: they live in L2).
// Per-band arrays are written straight into the unit's HeaacToolsFrame and read back from there, so the walk keeps no
// runtime-indexed private array; a quad codeword leaves as one 16-byte store, a pair as one 8-byte store.  The AAC
// calls are the same kernel with the SBR half compiled out, and the one-unit call heaac_aac_parse_device is that
// kernel with S = n, T = 1 and no taken / hold arrays: one lane per unit.
//
// k_parse_prep runs ahead of every walk in the same call: the tools, SBR and PS records zeroed and the SBR state rows
// copied in -> out, every lane of a wide grid, 16-byte stores between the unaligned ends of each array -- a kernel and
// not hipMemsetAsync (its graph node left the records unzeroed on replay with ROCm 7.0's runtime).
//
// Every device caller of pc_walk stands in this file and k_sbr_parse in k_parse.hip: with the callers of pc_walk and
// k_sbr_parse in one translation unit the compiler stopped inlining the readers (calls, and with them 60 bytes of
// scratch per lane).  Here the two instantiations are flattened, so each holds the whole walk in line.
//
// The same walk is instantiated for the host through pss_host: heaac_debug_aac_parse_core (T = 1),
// heaac_debug_aac_parse_core_streams / heaac_debug_heaac_parse_core_streams (include/heaac_debug.h).  parse_core.h is
// the one writing of the element syntax: the host parser (aac_parse.c) reads through the same pc_* functions with a
// PcHost record for its statuses, refusal progress and pulse data; the walk passes NULL and defers every such unit.
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
#include "k_copy.h"            // pz_zero, pz_copy

// tools[0 .. tools_words) = 0; sbr, ps likewise; st_out[0 .. st_words) = st_in[..] (0 words: not given)
__global__ __launch_bounds__(256) void k_parse_prep(uint32_t *tools, unsigned long long tools_words, const uint32_t *st_in,
                                                    uint32_t *st_out, unsigned long long st_words, uint32_t *sbr,
                                                    unsigned long long sbr_words, uint32_t *ps, unsigned long long ps_words)
{
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
    if (tools_words) pz_zero(tools, tools_words, gid, stride);
    if (st_words) pz_copy(st_out, st_in, st_words, gid, stride);
    if (sbr_words) pz_zero(sbr, sbr_words, gid, stride);
    if (ps_words) pz_zero(ps, ps_words, gid, stride);
}

// the grid by the largest of the counts: one 16-byte word per lane, grid-stride beyond 8 192 blocks
void heaac_launch_parse_prep(void *tools, unsigned long long tools_words, const void *st_in, void *st_out, unsigned long long st_words,
                             void *sbr, unsigned long long sbr_words, void *ps, unsigned long long ps_words, hipStream_t s)
{
    unsigned long long most = tools_words > st_words ? tools_words : st_words;
    most = most > sbr_words ? most : sbr_words;
    most = most > ps_words ? most : ps_words;
    unsigned long long pb = (most / 4 + 255) / 256;
    pb = pb < 1 ? 1 : pb > 8192 ? 8192 : pb;
    hipLaunchKernelGGL(k_parse_prep, dim3((unsigned)pb), dim3(256), 0, s, (uint32_t *)tools, tools_words, (const uint32_t *)st_in,
                       (uint32_t *)st_out, st_words, (uint32_t *)sbr, sbr_words, (uint32_t *)ps, ps_words);
}

template <int HE>
__global__ __launch_bounds__(PARSE_BLOCK) __attribute__((flatten)) void k_parse_streams(HeaacAacConfig cfg, const HeaacParseTables *t, const HeaacSbrParseTables *stab,
                                                               HeaacAacStream *st, const HeaacSbrStream *sst_in, HeaacSbrStream *sst_out,
                                                               const uint8_t *au, const uint32_t *au_offset, unsigned long long S,
                                                               uint32_t T, int coeff_channels, float *coeffs, HeaacIcs *ics,
                                                               HeaacToolsFrame *tools, HeaacAacFrameInfo *info, const HeaacSbrHeader *hdr,
                                                               uint32_t n_hdr, HeaacSbrFrame *sbr, HeaacPsFrame *ps, int32_t *status,
                                                               uint32_t *taken, uint8_t *hold)
{
    __shared__ uint4 s_lut[HEAAC_PT_BOOKS * HEAAC_PT_LUT / 4];
    __shared__ uint4 s_tab[HE ? sizeof(HeaacSbrParseTables) / 16 : 1];
    const uint4 *src = (const uint4 *)&t->lut[0][0];
    for (int k = threadIdx.x; k < HEAAC_PT_BOOKS * HEAAC_PT_LUT / 4; k += PARSE_BLOCK) s_lut[k] = src[k];
    if (HE) {
        const uint4 *ssrc = (const uint4 *)stab;
        for (int k = threadIdx.x; k < (int)(sizeof(HeaacSbrParseTables) / 16); k += PARSE_BLOCK) s_tab[k] = ssrc[k];
    }
    __syncthreads();
    const unsigned long long s = (unsigned long long)blockIdx.x * PARSE_BLOCK + threadIdx.x;
    if (s >= S) return;
    const size_t i = (size_t)s * T;
    pss_stream(&cfg, t, (const uint32_t *)s_lut, (const HeaacSbrParseTables *)s_tab, HE, st + s, HE ? sst_in + s : NULL,
               HE ? sst_out + s : NULL, au, au_offset + i, T, coeff_channels, coeffs + i * (size_t)coeff_channels * 1024,
               ics + i * (size_t)coeff_channels, tools + i, info + i, hdr, n_hdr, HE ? sbr + i : NULL, HE && ps ? ps + i : NULL,
               status + i, taken ? taken + s : NULL, hold ? hold + i : NULL, NULL);
}

// d_stab == NULL: the AAC calls (no SBR half, no state rows); d_taken and d_hold may be NULL
int heaac_launch_parse_streams(const HeaacParseTables *d_tab, const HeaacSbrParseTables *d_stab, const HeaacAacConfig *cfg,
                               HeaacAacStream *d_st, const HeaacSbrStream *d_sst_in, HeaacSbrStream *d_sst_out, const uint8_t *d_au,
                               const uint32_t *d_au_offset, size_t S, size_t T, int coeff_channels, float *d_coeffs, HeaacIcs *d_ics,
                               HeaacToolsFrame *d_tools, HeaacAacFrameInfo *d_info, const HeaacSbrHeader *d_hdr, size_t n_hdr,
                               HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps, int32_t *d_status, uint32_t *d_taken, uint8_t *d_hold,
                               hipStream_t s)
{
    if (S > PARSE_GRID_MAX || T > 0x7fffffffull) return HEAAC_ERR_ARG;
    const unsigned long long blocks = ((unsigned long long)S + PARSE_BLOCK - 1) / PARSE_BLOCK;
    const unsigned long long n = (unsigned long long)S * T;
    const unsigned long long tools_words = n * (sizeof(HeaacToolsFrame) / 4);
    const unsigned long long st_words = d_stab ? (unsigned long long)S * (sizeof(HeaacSbrStream) / 4) : 0ull;
    heaac_launch_parse_prep(d_tools, tools_words, d_sst_in, d_sst_out, st_words, d_sbr, d_stab ? n * (sizeof(HeaacSbrFrame) / 4) : 0ull,
                            d_ps, d_stab && d_ps ? n * (sizeof(HeaacPsFrame) / 4) : 0ull, s);
    const uint32_t nh = (uint32_t)(n_hdr > 0xffffffffull ? 0xffffffffull : n_hdr);
    if (d_stab)
        hipLaunchKernelGGL(k_parse_streams<1>, dim3((unsigned)blocks), dim3(PARSE_BLOCK), 0, s, *cfg, d_tab, d_stab, d_st, d_sst_in,
                           d_sst_out, d_au, d_au_offset, (unsigned long long)S, (uint32_t)T, coeff_channels, d_coeffs, d_ics, d_tools,
                           d_info, d_hdr, nh, d_sbr, d_ps, d_status, d_taken, d_hold);
    else
        hipLaunchKernelGGL(k_parse_streams<0>, dim3((unsigned)blocks), dim3(PARSE_BLOCK), 0, s, *cfg, d_tab, d_stab, d_st, d_sst_in,
                           d_sst_out, d_au, d_au_offset, (unsigned long long)S, (uint32_t)T, coeff_channels, d_coeffs, d_ics, d_tools,
                           d_info, d_hdr, nh, d_sbr, d_ps, d_status, d_taken, d_hold);
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

// heaac_aac_parse_device: n streams of one unit each.  The kernel indexes in 64 bits (s, s * T and every record offset
// are unsigned long long / size_t), so n is bounded by the grid alone (checked by the launcher below it), not by the
// streams calls' 32-bit unit index.
int heaac_launch_aac_parse(const HeaacParseTables *d_tab, const HeaacAacConfig *cfg, HeaacAacStream *d_st,
                           const uint8_t *d_au, const uint32_t *d_au_offset, size_t n, int coeff_channels,
                           float *d_coeffs, HeaacIcs *d_ics, HeaacToolsFrame *d_tools, HeaacAacFrameInfo *d_info,
                           int32_t *d_status, hipStream_t s)
{
    if (n > SIZE_MAX / sizeof(HeaacToolsFrame)) return HEAAC_ERR_ARG;
    return heaac_launch_parse_streams(d_tab, NULL, cfg, d_st, NULL, NULL, d_au, d_au_offset, n, 1, coeff_channels, d_coeffs, d_ics,
                                      d_tools, d_info, NULL, 0, NULL, NULL, d_status, NULL, NULL, s);
}

// what every form refuses before it looks at a unit
int heaac_parse_args_ok(const HeaacAacConfig *cfg, int coeff_channels)
{
    return cfg && coeff_channels >= 1 && coeff_channels <= 2 && cfg->sampling_index >= 0 && cfg->sampling_index <= 12 &&
           (cfg->object_type == HEAAC_AOT_AAC_LC || cfg->object_type == HEAAC_AOT_AAC_MAIN);
}

// The host form of the one-unit call: the chain at T = 1, one "stream" per unit.  There the reason of unit 0 is
// pc_walk's return, so `why` holds the PC_WHY_* values and PSS_WHY_STOPPED cannot occur (no unit stands behind t0).
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
    pss_host(cfg, t, NULL, 0, st, NULL, NULL, au, au_offset, n, 1, coeff_channels, coeffs, ics, tools, info, NULL, 0, NULL, NULL, status,
             NULL, NULL, why);
    return HEAAC_OK;
}

// What both streams calls, and their host forms, refuse for S > 0 (after heaac_parse_args_ok and T > 0): a NULL or
// misaligned pointer, an S * T beyond the grid or the record addressing, and for HE what heaac_sbr_parse_args_ok refuses
// (the state arrays are [S], the records [S * T]).
int heaac_parse_streams_args_ok(const HeaacAacConfig *cfg, int he, const void *st, const void *sst_in, const void *sst_out,
                                const void *au, const void *au_offset, size_t S, size_t T, const void *coeffs, const void *ics,
                                const void *tools, const void *info, const void *hdr, size_t n_hdr, const void *sbr, const void *ps,
                                const void *status, const void *taken)
{
    if (!cfg || T == 0 || T > 0x7fffffffull || S > PARSE_GRID_MAX || S > SIZE_MAX / T) return 0;
    const size_t n = S * T;
    // offsets are [n + 1] uint32_t; the widest record row is two coefficient rows (8 192 bytes)
    if (n > 0xfffffffeull || n > SIZE_MAX / (2 * 1024 * sizeof(float))) return 0;
    if (!st || !au || !au_offset || !coeffs || !ics || !tools || !info || !status || !taken) return 0;
    if (((uintptr_t)coeffs & 15) || (((uintptr_t)tools | (uintptr_t)au_offset | (uintptr_t)info | (uintptr_t)status | (uintptr_t)taken) & 3))
        return 0;
    if (he && !heaac_sbr_parse_args_ok(cfg, sst_in, sst_out, au, au_offset, info, S, hdr, n_hdr, sbr, ps, status)) return 0;
    return 1;
}

static int parse_core_streams(const HeaacAacConfig *cfg, int he, HeaacAacStream *st, const HeaacSbrStream *sst_in,
                              HeaacSbrStream *sst_out, const uint8_t *au, const uint32_t *au_offset, size_t S, size_t T,
                              int coeff_channels, float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools, HeaacAacFrameInfo *info,
                              const HeaacSbrHeader *hdr, size_t n_hdr, HeaacSbrFrame *sbr, HeaacPsFrame *ps, int32_t *status,
                              uint32_t *taken, uint8_t *hold, int32_t *why)
{
    if (!heaac_parse_args_ok(cfg, coeff_channels) || T == 0) return HEAAC_ERR_ARG;
    if (S == 0) return HEAAC_OK;
    if (!heaac_parse_streams_args_ok(cfg, he, st, sst_in, sst_out, au, au_offset, S, T, coeffs, ics, tools, info, hdr, n_hdr, sbr, ps,
                                     status, taken))
        return HEAAC_ERR_ARG;
    const HeaacParseTables *t = heaac_parse_tables();
    const HeaacSbrParseTables *stab = he ? heaac_sbr_parse_tables() : NULL;
    if (!t || (he && !stab)) return HEAAC_ERR_ARG;
    const uint32_t nh = (uint32_t)(n_hdr > 0xffffffffull ? 0xffffffffull : n_hdr);
    if (he)
        pss_host(cfg, t, stab, 1, st, sst_in, sst_out, au, au_offset, S, (uint32_t)T, coeff_channels, coeffs, ics, tools, info, hdr, nh,
                 sbr, ps, status, taken, hold, why);
    else
        pss_host(cfg, t, NULL, 0, st, NULL, NULL, au, au_offset, S, (uint32_t)T, coeff_channels, coeffs, ics, tools, info, NULL, 0, NULL,
                 NULL, status, taken, hold, why);
    return HEAAC_OK;
}

extern "C" int heaac_debug_aac_parse_core_streams(const HeaacAacConfig *cfg, HeaacAacStream *st, const uint8_t *au,
                                                  const uint32_t *au_offset, size_t n_streams, size_t frames_per_stream,
                                                  int coeff_channels, float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                                                  HeaacAacFrameInfo *info, int32_t *status, uint32_t *taken, uint8_t *hold,
                                                  int32_t *why)
{
    return parse_core_streams(cfg, 0, st, NULL, NULL, au, au_offset, n_streams, frames_per_stream, coeff_channels, coeffs, ics, tools,
                              info, NULL, 0, NULL, NULL, status, taken, hold, why);
}

extern "C" int heaac_debug_heaac_parse_core_streams(const HeaacAacConfig *cfg, HeaacAacStream *st, const HeaacSbrStream *sst_in,
                                                    HeaacSbrStream *sst_out, const uint8_t *au, const uint32_t *au_offset,
                                                    size_t n_streams, size_t frames_per_stream, int coeff_channels, float *coeffs,
                                                    HeaacIcs *ics, HeaacToolsFrame *tools, HeaacAacFrameInfo *info,
                                                    const HeaacSbrHeader *hdr, size_t n_hdr, HeaacSbrFrame *sbr, HeaacPsFrame *ps,
                                                    int32_t *status, uint32_t *taken, uint8_t *hold, int32_t *why)
{
    return parse_core_streams(cfg, 1, st, sst_in, sst_out, au, au_offset, n_streams, frames_per_stream, coeff_channels, coeffs, ics,
                              tools, info, hdr, n_hdr, sbr, ps, status, taken, hold, why);
}
