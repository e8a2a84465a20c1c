// k_copy.h -- device: fill and copy of 4-byte aligned arrays in 16-byte words between their unaligned ends, lanes
// gid, gid + stride, ...  (k_parse_prep of k_parse_streams.hip, the fix-up kernels of k_fix.hip).  64-bit counts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
