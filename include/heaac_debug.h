/* heaac_debug.h -- test-support entry points of libheaac_amd.so.  Not needed to use the library; declared so that
 * nothing the library exports is undeclared (the parity tests that poison the X hand-over workspace use this one:
 * tests/test_he_gpu.py::test_unstored_x_bands_are_never_read). */
#ifndef HEAAC_DEBUG_H
#define HEAAC_DEBUG_H

#include <stddef.h>
#include "heaac_dsp.h"
#include "heaac_parse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers of workspace set 0 of a device context -- W[chunk][2][32][32][2] floats (the analysis bank's output)
 * and X[chunk][2 channels][38][64][re, im] floats (the hand-over between the HF / PS kernels and the synthesis kernel)
 * -- and the chunk size in frames.  Any of the out pointers may be NULL.  The memory belongs to the context; what it
 * holds between calls is unspecified (the decode calls overwrite it), which is what a test that fills it with NaN
 * relies on.  Returns HEAAC_OK, or HEAAC_ERR_ARG for a NULL context. */
int heaac_debug_workspace(HeaacDevice *dev, float **d_W, float **d_X, size_t *chunk);

/* How many QMF bands of each X row the HF / PS stage stored for the frames of the LAST decode call (one byte per frame
 * and output channel: 32, 48 or 64; the bands above are +0 and the synthesis kernel reads them from a page of zeros --
 * DESIGN.md s4).  Copies 2 * n_frames bytes to host memory after a device synchronisation.  n_frames may be up to the
 * frames the context holds records for: its chunk (min(max_frames, 262144)) times its workspace sets (1, or the two
 * lanes where max_frames exceeds one chunk); more is HEAAC_ERR_ARG, as is a NULL context or buffer.  Chunk c of a
 * call leaves its records at byte 2 (c mod sets) chunk: for heaac_he_decode_batch(_ex) byte 2 f + ch is frame f,
 * channel ch.  heaac_he_decode_streams works in chunks of floor(chunk / T) whole streams, so its records are in frame
 * order only where T divides the chunk.  bench.py reports the shares, since the headline leans on them. */
int heaac_debug_xbands(HeaacDevice *dev, unsigned char *host_out, size_t n_frames);

/* The access-unit walk of heaac_aac_parse_device (csrc/parse_core.h) instantiated for the host: the same arguments
 * with host pointers, no device.  It is the chain of the streams form below at T = 1, one stream per unit (its own
 * argument checks, no `taken` / `hold`), as the device call is the streams kernel at T = 1.  The host parser reads the element syntax through the
 * same readers of csrc/parse_core.h; this is where the walk's deferrals and its commit-on-OK are compared with
 * heaac_aac_parse_frame_ex unit by unit, fuzzed and run under sanitizers, and where a kernel fault is debugged.
 * `why` (may be NULL) receives per unit 0 for HEAAC_PARSE_OK, or why the unit was deferred: 1 pulse data, 2 a CCE /
 * PCE / LFE or a second SCE / CPE, 4 a check of the host parser it does not pass (at T = 1 the chain's reason is the
 * walk's own; its "not looked at" value cannot occur). */
int heaac_debug_aac_parse_core(const HeaacAacConfig *cfg, HeaacAacStream *st, const uint8_t *au,
                               const uint32_t *au_offset, size_t n, int coeff_channels, float *coeffs,
                               HeaacIcs *ics, HeaacToolsFrame *tools, HeaacAacFrameInfo *info, int32_t *status,
                               int32_t *why);

/* The payload walk of heaac_sbr_parse_device (csrc/sbr_core.h) instantiated for the host: the same arguments with host
 * pointers, a plain loop over the n units, no device.  `why` (may be NULL) receives per unit 0 for HEAAC_PARSE_OK, or
 * why the unit was deferred: 1 a header that resets or touches the derived record, 2 the stream's header index is not
 * below n_hdr, 4 a misplaced payload, 8 the host parser would not return HEAAC_PARSE_OK, 16 the AAC status is not OK. */
int heaac_debug_sbr_parse_core(const HeaacAacConfig *cfg, const HeaacSbrStream *sst_in, HeaacSbrStream *sst_out,
                               const uint8_t *au, const uint32_t *au_offset, const HeaacAacFrameInfo *info,
                               const int32_t *aac_status, size_t n, const HeaacSbrHeader *hdr, size_t n_hdr,
                               HeaacSbrFrame *sbr, HeaacPsFrame *ps, int32_t *status, int32_t *why);

/* The chains of heaac_aac_parse_device_streams and heaac_heaac_parse_device_streams (csrc/parse_streams.h) instantiated
 * for the host: the same arguments with host pointers, the same argument checks, a plain loop over the streams, no
 * device.  `why` [S][T] (may be NULL) receives 0 for a unit that was taken; for the unit a stream stopped at the AAC
 * walk's reason (1, 2, 4 as above) or 256 times the SBR walk's reason (1 .. 8 as above); 1 << 20 for the units behind
 * it, which were not looked at. */
int heaac_debug_aac_parse_core_streams(const HeaacAacConfig *cfg, HeaacAacStream *st, const uint8_t *au,
                                       const uint32_t *au_offset, size_t n_streams, size_t frames_per_stream,
                                       int coeff_channels, float *coeffs, HeaacIcs *ics, HeaacToolsFrame *tools,
                                       HeaacAacFrameInfo *info, int32_t *status, uint32_t *taken, uint8_t *hold, int32_t *why);
int heaac_debug_heaac_parse_core_streams(const HeaacAacConfig *cfg, HeaacAacStream *st, const HeaacSbrStream *sst_in,
                                         HeaacSbrStream *sst_out, const uint8_t *au, const uint32_t *au_offset,
                                         size_t n_streams, size_t frames_per_stream, int coeff_channels, float *coeffs,
                                         HeaacIcs *ics, HeaacToolsFrame *tools, HeaacAacFrameInfo *info,
                                         const HeaacSbrHeader *hdr, size_t n_hdr, HeaacSbrFrame *sbr, HeaacPsFrame *ps,
                                         int32_t *status, uint32_t *taken, uint8_t *hold, int32_t *why);

/* The two host steps of a device-parse tick of heaac_pipeline_* that are plain C (csrc/pipeline_pack.h), as submit runs
 * them.  pack: offset [n_units + 1] of the units laid end to end, a unit with size <= 0 an empty one (its pointer is not
 * looked at), and -- unless bytes is NULL -- their bytes copied to bytes[offset[i] ...]; with bytes == NULL nothing but
 * size[] is read and au may be NULL.  HEAAC_ERR_ARG where the tick's bytes do not fit 32-bit offsets, before a byte is
 * copied.  stops: taken [n_streams] (t0 per stream, as the streams walk writes it) -> the streams with t0 < T in
 * ascending order in list [n_streams], and in base [n_streams + 1] where each one's unit t0 stands among the units
 * handed to the host parser (base[m] = their count); returns m. */
int heaac_debug_pipeline_pack(const uint8_t *const *au, const int *size, size_t n_units, uint8_t *bytes, uint32_t *offset);
size_t heaac_debug_pipeline_stops(const uint32_t *taken, size_t n_streams, size_t frames_per_tick, uint32_t *list,
                                  uint32_t *base);

#ifdef __cplusplus
}
#endif
#endif /* HEAAC_DEBUG_H */
