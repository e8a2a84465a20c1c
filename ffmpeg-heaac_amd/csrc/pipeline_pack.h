/* pipeline_pack.h -- the two host steps of a device-parse tick of heaac_pipeline_* (pipeline.hip) that touch the
 * caller's buffers and the walk's answer: packing the tick's access units into one byte buffer with 32-bit offsets,
 * and turning the walk's `taken` array into the list of streams the host parser has to finish.  Plain C, no HIP and no
 * library state, so that it builds stand-alone: tests/c/pipeline_pack.c runs it under sanitizers with every unit at
 * the end of its heap block, and heaac_debug_pipeline_pack / heaac_debug_pipeline_stops (include/heaac_debug.h) hand it
 * to the tests.
 */
#ifndef HEAAC_PIPELINE_PACK_H
#define HEAAC_PIPELINE_PACK_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* offset[0 .. n] of n units laid end to end: unit i is bytes [offset[i], offset[i + 1]).  A unit with size <= 0 is an
 * empty unit (the device walk defers it, and the host parser then answers HEAAC_PARSE_ERR_ARG).  Returns 0, or -1 where
 * the bytes of the tick do not fit 32-bit offsets (offset[] is then unspecified).  Reads size[] only. */
static inline int heaac_pack_offsets(const int *size, size_t n, uint32_t *offset)
{
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        offset[i] = (uint32_t)at;
        if (size[i] > 0) at += (uint64_t)size[i];
        if (at > 0xffffffffull) return -1;
    }
    offset[n] = (uint32_t)at;
    return 0;
}

/* The bytes of the units [lo, hi) to their places in dst (one slice of the pool); a unit of size <= 0 is not looked
 * at, so its pointer may be anything. */
static inline void heaac_pack_bytes(const uint8_t *const *au, const int *size, const uint32_t *offset, size_t lo, size_t hi,
                                    uint8_t *dst)
{
    for (size_t i = lo; i < hi; i++)
        if (size[i] > 0) memcpy(dst + offset[i], au[i], (size_t)size[i]);
}

/* taken[n] (t0 of each stream, T where the walk took all of its units) -> the streams with t0 < T in ascending order:
 * list[j] is the j-th such stream and base[j] the place of its unit t0 among the units the host parser is handed, which
 * are numbered stream by stream; base[m] is their count.  list [n], base [n + 1].  Returns m.  A t0 above T counts as
 * T. */
static inline size_t heaac_stop_list(const uint32_t *taken, size_t n, uint32_t T, uint32_t *list, uint32_t *base)
{
    size_t m = 0;
    uint32_t units = 0;
    for (size_t s = 0; s < n; s++) {
        if (taken[s] >= T) continue;
        list[m] = (uint32_t)s;
        base[m] = units;
        units += T - taken[s];
        m++;
    }
    base[m] = units;
    return m;
}

#endif /* HEAAC_PIPELINE_PACK_H */
