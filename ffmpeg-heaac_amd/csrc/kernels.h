// kernels.h -- internal launch functions (one per .hip translation unit).
// Not part of the public ABI; include/heaac_dsp.h is.
// d_hold: the [S][T] hold mask of the *_streams_ex calls (NULL: none, the kernels of the plain calls run).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "heaac_dsp.h"

extern "C" {
/* n_streams x frames_per_stream frames; one frame per stream without a mask runs the batch kernel */
int heaac_launch_lc(const float *d_tab, const uint16_t *d_rev, int channels,
                    const float *d_coeffs, const HeaacIcs *d_ics,
                    const float *d_state_in, float *d_state_out,
                    void *d_pcm, int pcm_format, size_t n_streams, size_t frames_per_stream,
                    const uint8_t *d_hold, hipStream_t s);

int heaac_launch_imdct_half(const float *d_tab, const uint16_t *d_rev, int which,
                            float *d_out, const float *d_in, size_t n, hipStream_t s);

int heaac_launch_couple(int channels, float *d_pcm, const float *d_cce, const HeaacCoupling *d_cpl,
                        int16_t *d_s16, size_t n, hipStream_t s);

int heaac_launch_interleave(int channels, const HeaacPlaneRef *planes, int len, int pcm_format, int16_t *d_out,
                            size_t n, hipStream_t s);

/* One HE call over a chunk of whole streams: everything heaac_launch_he reads.  Frame (s, t) is record s * T + t of the
 * per-frame arrays; the state is one record per stream.  T == 1 without a mask runs the batch kernels. */
struct HeaacHeLaunch {
    const float *d_tab;                 /* tables */
    const uint16_t *d_rev;
    int cfg, flags;                     /* HEAAC_CFG_*, HEAAC_HE_* */
    const HeaacSbrHeader *d_hdr;
    unsigned n_hdr;
    const float *d_coeffs;              /* per frame */
    const HeaacIcs *d_ics;
    const HeaacSbrFrame *d_sbr;
    const HeaacPsFrame *d_ps;           /* HE-AACv2 only */
    const float *d_state_in;            /* per stream */
    float *d_state_out;
    void *d_pcm;
    int pcm_format;
    float *d_ws_W, *d_ws_X;             /* one workspace set: W / X hand-over, queue heads, X band counts, zero page */
    unsigned *d_queue;
    unsigned char *d_xtop;
    const float *d_zero;
    size_t n_streams, T;
    const uint8_t *d_hold;
    hipStream_t s;
};
int heaac_launch_he(const struct HeaacHeLaunch *a);

/* k_ps.hip: the HE-AACv2 launches of heaac_launch_he for position t of its streams (st_in: the state frame t reads) */
int heaac_launch_hfps(const struct HeaacHeLaunch *a, size_t t, const float *st_in, const float *W, float *X);
int heaac_launch_ps(const struct HeaacHeLaunch *a, size_t t, const float *st_in, float *X);

int heaac_launch_qmf_analysis(const float *d_tab, const float *d_in, const float *d_xh_in,
                              float *d_xh_out, float *d_W, float scale, size_t n, hipStream_t s);

int heaac_launch_qmf_synthesis(const float *d_tab, const float *d_X, const float *d_v_in,
                               float *d_v_out, float *d_out, float scale, float bias,
                               size_t n, hipStream_t s);

int heaac_launch_qmf_synthesis_ds(const float *d_tab, const float *d_X, const float *d_v_in,
                                  float *d_v_out, float *d_out, float scale, float bias,
                                  size_t n, hipStream_t s);

int heaac_launch_spectral_tools(int channels, float *d_coeffs, const HeaacToolsFrame *d_tools,
                                const int *d_rng_in, int *d_rng_out,
                                const HeaacPredictorState *d_pred_in, HeaacPredictorState *d_pred_out,
                                int stages, const HeaacCceFrame *d_cce, const float *d_cce_coeffs, int n_cce,
                                size_t n, hipStream_t s);

/* one frame per stream, or no state at all, is one call of the batch launcher -- never with a mask */
int heaac_launch_spectral_tools_streams(int channels, float *d_coeffs, const HeaacToolsFrame *d_tools,
                                        const int *d_rng_in, int *d_rng_out,
                                        const HeaacPredictorState *d_pred_in, HeaacPredictorState *d_pred_out,
                                        size_t n_streams, size_t frames_per_stream, const uint8_t *d_hold,
                                        hipStream_t s);
int heaac_launch_fft_calc(const float *d_tab, int nbits, float *d_z, size_t n, hipStream_t s);
int heaac_launch_imdct_mirror(float *d_out, int n, size_t count, hipStream_t s);

/* k_parse_streams.hip: heaac_aac_parse_device (include/heaac_parse.h), the streams launcher below with S = n, T = 1;
 * d_tab = the device copy of heaac_parse_tables() */
struct HeaacParseTables;
struct HeaacAacConfig;
struct HeaacAacStream;
struct HeaacAacFrameInfo;
int heaac_parse_args_ok(const struct HeaacAacConfig *cfg, int coeff_channels);
int heaac_launch_aac_parse(const struct HeaacParseTables *d_tab, const struct HeaacAacConfig *cfg, struct HeaacAacStream *d_st,
                           const uint8_t *d_au, const uint32_t *d_au_offset, size_t n, int coeff_channels,
                           float *d_coeffs, HeaacIcs *d_ics, HeaacToolsFrame *d_tools, struct HeaacAacFrameInfo *d_info,
                           int32_t *d_status, hipStream_t s);

/* k_parse.hip: heaac_sbr_parse_device; d_tab = the device copy of heaac_sbr_parse_tables() (sbr_core.h) */
struct HeaacSbrParseTables;
struct HeaacSbrStream;
int heaac_sbr_parse_args_ok(const struct HeaacAacConfig *cfg, const void *sst_in, const void *sst_out, const void *au,
                            const void *au_offset, const void *info, size_t n, const void *hdr, size_t n_hdr, const void *sbr,
                            const void *ps, const void *status);
int heaac_launch_sbr_parse(const struct HeaacSbrParseTables *d_tab, const struct HeaacAacConfig *cfg,
                           const struct HeaacSbrStream *d_sst_in, struct HeaacSbrStream *d_sst_out, const uint8_t *d_au,
                           const uint32_t *d_au_offset, const struct HeaacAacFrameInfo *d_info, const int32_t *d_aac_status,
                           size_t n, const HeaacSbrHeader *d_hdr, size_t n_hdr, HeaacSbrFrame *d_sbr, HeaacPsFrame *d_ps,
                           int32_t *d_status, hipStream_t s);

/* k_parse_streams.hip: heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams (csrc/parse_streams.h): S
 * streams x T units, one lane per stream behind the prep kernel; d_stab == NULL launches the walk without its SBR half;
 * d_taken, d_hold may be NULL */
int heaac_parse_streams_args_ok(const struct HeaacAacConfig *cfg, int he, const void *st, const void *sst_in, const void *sst_out,
                                const void *au, const void *au_offset, size_t S, size_t T, const void *coeffs, const void *ics,
                                const void *tools, const void *info, const void *hdr, size_t n_hdr, const void *sbr, const void *ps,
                                const void *status, const void *taken);
int heaac_launch_parse_streams(const struct HeaacParseTables *d_tab, const struct HeaacSbrParseTables *d_stab,
                               const struct HeaacAacConfig *cfg, struct HeaacAacStream *d_st, const struct HeaacSbrStream *d_sst_in,
                               struct HeaacSbrStream *d_sst_out, const uint8_t *d_au, const uint32_t *d_au_offset, size_t S, size_t T,
                               int coeff_channels, float *d_coeffs, HeaacIcs *d_ics, HeaacToolsFrame *d_tools,
                               struct HeaacAacFrameInfo *d_info, const HeaacSbrHeader *d_hdr, size_t n_hdr, HeaacSbrFrame *d_sbr,
                               HeaacPsFrame *d_ps, int32_t *d_status, uint32_t *d_taken, uint8_t *d_hold, hipStream_t s);
}
