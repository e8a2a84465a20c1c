// k_parse_streams.hip -- heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams: the chain of parse_streams.h,
// one lane per STREAM.
//
// k_parse_streams<HE>: 64 streams per wave, one wave per block; the lane loops over its T units, pc_walk and then (HE)
// sc_walk per unit, each from the state the unit before left, and stops at the first unit either gives up.  The twelve
// prefix tables of k_aac_parse (48 KB) and, for HE, the 3 520 bytes of SBR / PS code-book nodes are copied to LDS at
// the head of the block.  The AAC call is the same kernel with the SBR half compiled out.  k_parse_streams_prep runs
// ahead of it in the same call: the S*T tools, SBR and PS records zeroed and the S state rows copied in -> out, every
// lane of a wide grid, 16-byte stores (a kernel and not hipMemsetAsync).
//
// The kernels stand in a file of their own: with a second caller of pc_walk in k_parse.hip the compiler stopped
// inlining the readers into k_aac_parse (calls, and with them 60 bytes of scratch per lane).  Here the two
// instantiations are flattened, so each holds the whole walk in line as k_aac_parse does.
//
// heaac_debug_aac_parse_core_streams / heaac_debug_heaac_parse_core_streams are the host forms (include/heaac_debug.h).
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

#define PARSE_BLOCK 64

// p[0 .. words) = 0, 16-byte stores between the unaligned ends; p is 4-byte aligned
static __device__ inline void pz_zero(uint32_t *p, unsigned long long words, unsigned long long gid, unsigned long long stride)
{
    unsigned long long head = ((16 - ((uintptr_t)p & 15)) & 15) >> 2;
    if (head > words) head = words;
    const unsigned long long body = (words - head) >> 2, tail = (words - head) & 3;
    uint4 *q = (uint4 *)(p + head);
    if (gid < head) p[gid] = 0;
    for (unsigned long long k = gid; k < body; k += stride) q[k] = make_uint4(0, 0, 0, 0);
    if (gid < tail) p[head + body * 4 + gid] = 0;
}

// d[0 .. words) = s[..]; 16-byte words where the two share their alignment, else 4-byte ones
static __device__ inline void pz_copy(uint32_t *d, const uint32_t *s, unsigned long long words, unsigned long long gid,
                                      unsigned long long stride)
{
    if ((((uintptr_t)d ^ (uintptr_t)s) & 15) != 0) {
        for (unsigned long long k = gid; k < words; k += stride) d[k] = s[k];
        return;
    }
    unsigned long long head = ((16 - ((uintptr_t)d & 15)) & 15) >> 2;
    if (head > words) head = words;
    const unsigned long long body = (words - head) >> 2, tail = (words - head) & 3;
    const uint4 *qs = (const uint4 *)(s + head);
    uint4 *qd = (uint4 *)(d + head);
    if (gid < head) d[gid] = s[gid];
    for (unsigned long long k = gid; k < body; k += stride) qd[k] = qs[k];
    if (gid < tail) d[head + body * 4 + gid] = s[head + body * 4 + gid];
}

// tools[0 .. tools_words) = 0; sbr, ps likewise (0 words: not given); st_out[0 .. st_words) = st_in[..]
__global__ __launch_bounds__(256) void k_parse_streams_prep(uint32_t *tools, unsigned long long tools_words, const uint32_t *st_in,
                                                            uint32_t *st_out, unsigned long long st_words, uint32_t *sbr,
                                                            unsigned long long sbr_words, uint32_t *ps, unsigned long long ps_words)
{
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, stride = (unsigned long long)gridDim.x * 256;
    pz_zero(tools, tools_words, gid, stride);
    if (st_words) pz_copy(st_out, st_in, st_words, gid, stride);
    if (sbr_words) pz_zero(sbr, sbr_words, gid, stride);
    if (ps_words) pz_zero(ps, ps_words, gid, stride);
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
               status + i, taken + s, hold ? hold + i : NULL, NULL);
}

// d_stab == NULL: the AAC call (no SBR half, no state rows)
int heaac_launch_parse_streams(const HeaacParseTables *d_tab, const HeaacSbrParseTables *d_stab, const HeaacAacConfig *cfg,
                               HeaacAacStream *d_st, const HeaacSbrStream *d_sst_in, HeaacSbrStream *d_sst_out, const uint8_t *d_au,
                               const uint32_t *d_au_offset, size_t S, size_t T, int coeff_channels, float *d_coeffs, HeaacIcs *d_ics,
                               HeaacToolsFrame *d_tools, HeaacAacFrameInfo *d_info, const HeaacSbrHeader *d_hdr, size_t n_hdr,
                               HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps, int32_t *d_status, uint32_t *d_taken, uint8_t *d_hold,
                               hipStream_t s)
{
    const unsigned long long blocks = ((unsigned long long)S + PARSE_BLOCK - 1) / PARSE_BLOCK;
    if (blocks > 0x7fffffffull || T > 0x7fffffffull) return HEAAC_ERR_ARG;
    const unsigned long long n = (unsigned long long)S * T;
    const unsigned long long tools_words = n * (sizeof(HeaacToolsFrame) / 4);
    const unsigned long long st_words = d_stab ? (unsigned long long)S * (sizeof(HeaacSbrStream) / 4) : 0ull;
    unsigned long long pb = (tools_words / 4 + 255) / 256;
    pb = pb < 1 ? 1 : pb > 8192 ? 8192 : pb;
    hipLaunchKernelGGL(k_parse_streams_prep, dim3((unsigned)pb), dim3(256), 0, s, (uint32_t *)d_tools, tools_words,
                       (const uint32_t *)d_sst_in, (uint32_t *)d_sst_out, st_words, (uint32_t *)d_sbr,
                       d_stab ? n * (sizeof(HeaacSbrFrame) / 4) : 0ull, (uint32_t *)d_ps,
                       d_stab && d_ps ? n * (sizeof(HeaacPsFrame) / 4) : 0ull);
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

// What both streams calls, and their host forms, refuse for S > 0 (after heaac_parse_args_ok and T > 0): a NULL or
// misaligned pointer, an S * T beyond the grid or the record addressing, and for HE what heaac_sbr_parse_args_ok refuses
// (the state arrays are [S], the records [S * T]).
int heaac_parse_streams_args_ok(const HeaacAacConfig *cfg, int he, const void *st, const void *sst_in, const void *sst_out,
                                const void *au, const void *au_offset, size_t S, size_t T, const void *coeffs, const void *ics,
                                const void *tools, const void *info, const void *hdr, size_t n_hdr, const void *sbr, const void *ps,
                                const void *status, const void *taken)
{
    if (!cfg || T == 0 || T > 0x7fffffffull || S > 0x7fffffffull * PARSE_BLOCK || S > SIZE_MAX / T) return 0;
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
