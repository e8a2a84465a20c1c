// k_fix.hip -- the kernels of a device-parse tick of heaac_pipeline_* (pipeline.hip) around the walk of
// k_parse_streams.hip, all on the pipeline's `in` stream:
//
//   k_parse_status  behind the walk: the walk's HEAAC_PARSE_OK becomes the status the host parser would have returned
//                   for the unit (HEAAC_PARSE_NO_SBR where an HE unit carried no payload, read from sbr_payload_bit as
//                   heaac_sbr_parse_device's contract says), stored straight into the pipeline's pinned host array where
//                   the caller asked for statuses; and the tick's hold_tools mask is cleared: a unit the walk took is
//                   never held, and the fix-up writes the bytes of the others.
//   k_fix_gather    the AAC and SBR parser state rows of the m streams the walk stopped -> a compact buffer in pinned
//                   host memory the host parser resumes from.
//   k_fix_scatter   what the host parser made of those streams' remaining units: every staged record row to row
//                   s T + t of the tick's arrays, the two hold bytes to the tick's masks, the state rows back.
// What submit waits for -- the stop positions, the statuses, the gathered rows -- is stored by the kernels into mapped
// host memory (a few bytes per stream in the usual tick) instead of being copied back by commands of their own behind
// the kernels; the end-to-end rate measured the same either way.
//
// Plain copy kernels: one block of 256 lanes per staged unit or state row, rows moved by pz_copy (k_copy.h: 16-byte
// words where source and destination share their alignment -- always for the coefficient rows, and for every row of a
// stream's first HE tick, where the whole tick is staged in place order --, 4-byte words otherwise), 64-bit offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "heaac_dsp.h"
#include "heaac_parse.h"
#include "host_common.h"
#include "k_copy.h"

#define FIX_BLOCK 256

__global__ __launch_bounds__(FIX_BLOCK) void k_parse_status(const int32_t *status, const HeaacAacFrameInfo *info, int he, int sbr_off,
                                                            int32_t *host_status, uint8_t *hold_tools, unsigned long long nf)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * FIX_BLOCK + threadIdx.x;
    if (i >= nf) return;
    hold_tools[i] = 0;
    if (!host_status) return;
    int32_t r = status[i];
    if (he && r == HEAAC_PARSE_OK && (sbr_off || info[i].sbr_payload_bit < 0)) r = HEAAC_PARSE_NO_SBR;
    host_status[i] = r;
}

__global__ __launch_bounds__(FIX_BLOCK) void k_fix_gather(const uint32_t *list, const uint32_t *ast, uint32_t *g_ast,
                                                          uint32_t ast_words, const uint32_t *sst, uint32_t *g_sst,
                                                          uint32_t sst_words)
{
    const unsigned long long j = blockIdx.x, s = list[j];
    pz_copy(g_ast + j * ast_words, ast + s * ast_words, ast_words, threadIdx.x, FIX_BLOCK);
    if (sst_words) pz_copy(g_sst + j * sst_words, sst + s * sst_words, sst_words, threadIdx.x, FIX_BLOCK);
}

__global__ __launch_bounds__(FIX_BLOCK) void k_fix_scatter(HeaacFixRows a, const uint32_t *dest, uint32_t units,
                                                           const uint8_t *staged_hold, uint8_t *hold, unsigned long long nf,
                                                           const uint32_t *list, const uint32_t *g_ast, uint32_t *ast,
                                                           uint32_t ast_words, const uint32_t *g_sst, uint32_t *sst,
                                                           uint32_t sst_words)
{
    const unsigned long long b = blockIdx.x;
    if (b < units) {
        const unsigned long long r = dest[b];
        for (int k = 0; k < HEAAC_FIX_ARRAYS; k++) {
            const unsigned long long w = a.words[k];
            if (w) pz_copy(a.dst[k] + r * w, a.src[k] + b * w, w, threadIdx.x, FIX_BLOCK);
        }
        if (threadIdx.x == 0) {
            hold[r] = staged_hold[b];
            hold[nf + r] = staged_hold[units + b];
        }
        return;
    }
    const unsigned long long j = b - units, s = list[j];
    pz_copy(ast + s * ast_words, g_ast + j * ast_words, ast_words, threadIdx.x, FIX_BLOCK);
    if (sst_words) pz_copy(sst + s * sst_words, g_sst + j * sst_words, sst_words, threadIdx.x, FIX_BLOCK);
}

int heaac_launch_parse_status(hipStream_t s, const int32_t *d_status, const HeaacAacFrameInfo *d_info, int he, int sbr_off,
                              int32_t *host_status, uint8_t *d_hold_tools, size_t nf)
{
    const unsigned long long blocks = ((unsigned long long)nf + FIX_BLOCK - 1) / FIX_BLOCK;
    if (!nf || blocks > 0x7fffffffull) return HEAAC_ERR_ARG;
    hipLaunchKernelGGL(k_parse_status, dim3((unsigned)blocks), dim3(FIX_BLOCK), 0, s, d_status, d_info, he, sbr_off, host_status,
                       d_hold_tools, (unsigned long long)nf);
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

int heaac_launch_fix_gather(hipStream_t s, const uint32_t *d_list, size_t m, const HeaacAacStream *d_ast, void *d_g_ast,
                            const HeaacSbrStream *d_sst, void *d_g_sst)
{
    if (!m || m > 0x7fffffffull) return HEAAC_ERR_ARG;
    hipLaunchKernelGGL(k_fix_gather, dim3((unsigned)m), dim3(FIX_BLOCK), 0, s, d_list, (const uint32_t *)d_ast, (uint32_t *)d_g_ast,
                       (uint32_t)(sizeof(HeaacAacStream) / 4), (const uint32_t *)d_sst, (uint32_t *)d_g_sst,
                       (uint32_t)(d_sst ? sizeof(HeaacSbrStream) / 4 : 0));
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

int heaac_launch_fix_scatter(hipStream_t s, const HeaacFixRows *rows, const uint32_t *d_dest, size_t units,
                             const uint8_t *d_staged_hold, uint8_t *d_hold, size_t nf, const uint32_t *d_list, size_t m,
                             const void *d_g_ast, HeaacAacStream *d_ast, const void *d_g_sst, HeaacSbrStream *d_sst)
{
    if (!m || !units || (unsigned long long)units + m > 0x7fffffffull) return HEAAC_ERR_ARG;
    hipLaunchKernelGGL(k_fix_scatter, dim3((unsigned)(units + m)), dim3(FIX_BLOCK), 0, s, *rows, d_dest, (uint32_t)units, d_staged_hold,
                       d_hold, (unsigned long long)nf, d_list, (const uint32_t *)d_g_ast, (uint32_t *)d_ast,
                       (uint32_t)(sizeof(HeaacAacStream) / 4), (const uint32_t *)d_g_sst, (uint32_t *)d_sst,
                       (uint32_t)(d_sst ? sizeof(HeaacSbrStream) / 4 : 0));
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}
