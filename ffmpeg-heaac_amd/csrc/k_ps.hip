// k_ps.hip -- Parametric Stereo kernels for gfx950: ff_ps_apply() (aacps.c:973-992) =
// hybrid_analysis (:359-395), decorrelation (:645-754), stereo_processing (:794-971),
// hybrid_synthesis (:397-445), one wavefront per frame (device code: k_psf.h).
//
//   k_hfps         HF adjustment (k_hf.h) fused with baseline PS (20 bands, no IPD/OPD): the HE-AACv2 hot path
//   k_ps<true,5>   every other layout: 34 bands, IPD/OPD, 20 <-> 34 switches, PS off
//
// Lane = frequency band.  Every recursion of the reference (transient smoother, all-pass chain,
// H-matrix interpolation) runs over time inside one lane, so the reference's operation order is
// kept and parallelism comes from the 71 / 91 hybrid bands.  Plain QMF bands are columns held in
// registers; the hybrid sub-subbands of the lowest 3 / 5 QMF bands are kept in LDS.
#include "k_common.h"
#include "kernels.h"
#include "host_common.h"

#include "k_hf.h"
#include "k_psf.h"

// STRIDED (heaac_he_decode_streams): frame f's SBR and PS records are at f * rstride; X and state at f.
// Hold (heaac_he_decode_streams_ex; STRIDED only; k_common.h hold_mask): byte f * rstride != 0 -- frame f is nobody's,
// its records are not read.
template <bool GENERAL, int WAVES, bool STRIDED = false, class... Hold>
__global__ __launch_bounds__(WAVES * WAVE)
void k_ps(const float *__restrict__ g_tab, const HeaacPsFrame *__restrict__ g_ps,
          const HeaacSbrFrame *__restrict__ g_sbr, const HeaacSbrHeader *__restrict__ g_hdr, unsigned n_hdr,
          const float *g_state_in, float *g_state_out, int state_words, int off_ps,
          float *g_X, unsigned long long n, unsigned long long rstride, Hold... hold)
{
    static_assert(STRIDED || sizeof...(Hold) == 0, "the batch form has no hold mask");
    using WT = PsWaveT<GENERAL>;
    __shared__ HeaacPsFrame s_p[WAVES];
    __shared__ float s_inb[WAVES][WT::NLOW][44][2];
    __shared__ float s_scr[WAVES][WT::SCR];          // |s|^2, later subL / subR
    __shared__ float s_sub[WAVES][WT::SUBROWS][SUB_STRIDE];
    __shared__ float s_pw[WAVES][WT::NPAR][33];
    __shared__ float s_Hs[WAVES][6][WT::NH][WT::NPAR];
    // IPD/OPD index rows exist only in the general variant (the baseline one never touches them)
    __shared__ signed char s_idx[WAVES][GENERAL ? 4 : 2][5][WT::NPAR];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE;
    // mixed sub-subband outputs: baseline = two blocks in the scratch; general = left in place over the sub-subband
    // rows, right in the scratch
    WT W = { s_p[wave], s_inb[wave], s_scr[wave], s_sub[wave],
             GENERAL ? s_sub[wave] : reinterpret_cast<float (*)[SUB_STRIDE]>(s_scr[wave]),
             reinterpret_cast<float (*)[SUB_STRIDE]>(s_scr[wave] + (GENERAL ? 0 : (WT::NSUB + 1) * SUB_STRIDE)),
             s_pw[wave], s_Hs[wave], s_idx[wave][0], s_idx[wave][1],
             s_idx[wave][GENERAL ? 2 : 0], s_idx[wave][GENERAL ? 3 : 0],
             g_tab + TB_F20_0_8, g_tab + TB_G1_Q2 };
    const v2f no_cols[32] = {};
    // Frames are dealt round-robin to the waves of the grid; a wave checks the ownership of its
    // next 64 frames at once (one per lane), so a launch that owns few frames costs microseconds.
    const unsigned long long wid = (unsigned long long)blockIdx.x * WAVES + wave;
    const unsigned long long nw = (unsigned long long)gridDim.x * WAVES;
    for (unsigned long long base = wid; base < n; base += nw * WAVE) {
        const unsigned long long fl = base + (unsigned long long)lane * nw;
        bool mine;
        if constexpr (sizeof...(Hold) != 0)
            mine = fl < n && !hold_mask(hold...)[fl * rstride] && ps_frame_is_general(&g_ps[fl * rstride]) == GENERAL;
        else
            mine = fl < n && ps_frame_is_general(&g_ps[STRIDED ? fl * rstride : fl]) == GENERAL;
        unsigned long long todo = __ballot(mine);
        while (todo) {
            const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
            todo &= todo - 1;
            const unsigned long long f = base + (unsigned long long)j * nw, rf = STRIDED ? f * rstride : f;
            const unsigned hi = g_sbr[rf].hdr;
            const HeaacSbrHeader &h = g_hdr[hi < n_hdr ? hi : n_hdr - 1];
            const int top = h.kx + h.m;             // ff_ps_apply(..., sbr->kx[1] + sbr->m[1])
            float *XL = g_X + (f * 2) * HE_X_CHANNEL;
            ps_frame<GENERAL>(W, g_tab, &g_ps[rf], top, g_state_in + f * state_words + off_ps,
                              g_state_out + f * state_words + off_ps, XL, lane, wave, no_cols);
        }
    }
}

// ---------------------------------------------------------------------------
// Fused HF adjustment + Parametric Stereo for HE-AACv2 (mono core): the wave that
// finishes sbr_x_gen for a frame keeps X[.][0..31][k] of its band k in registers and
// runs ff_ps_apply on it, so the mono QMF signal never travels through HBM.  The HF
// stage's LDS (X_low, limiter sums, side info) is dead by then and is laid under the PS
// arrays.  Frames whose PS layout is not the baseline one (34 bands, IPD/OPD, PS off)
// get X written out and are finished by k_ps<true>.
// ---------------------------------------------------------------------------
#define HFPS_WAVES 8
#define HFPS_QUEUE_CHUNK 1      // frames per queue ticket
#define HFPS_C_WORDS (HF_REC_WORDS > 20 * 33 ? HF_REC_WORDS : 20 * 33)

// STRIDED (heaac_he_decode_streams): frame f's SBR and PS records are at f * rstride; W, X, xtop and state at f.
// Hold (heaac_he_decode_streams_ex; STRIDED only; k_common.h hold_mask): byte f * rstride != 0 -- frame f is passed over
// like one that is another kernel's; its records are not read (the look-ahead may touch them into L2: no value is used).
template <bool STRIDED, class... Hold>
__global__ __launch_bounds__(HFPS_WAVES * WAVE)
void k_hfps(const float *__restrict__ g_tab, const HeaacSbrFrame *__restrict__ g_sbr,
            const HeaacSbrHeader *__restrict__ g_hdr, unsigned n_hdr, const HeaacPsFrame *__restrict__ g_ps,
            const float *g_W, const float *g_state_in, float *g_state_out, int state_words,
            int off_sbr, int off_ps, float *g_X, unsigned long long n_frames, unsigned *g_queue,
            unsigned char *__restrict__ g_xtop, int skip_fast, unsigned long long rstride, Hold... hold)
{
    static_assert(STRIDED || sizeof...(Hold) == 0, "the batch form has no hold mask");
    using WT = PsWaveT<false>;
    static_assert(WT::SCR <= HF_XLOW_WORDS, "|s|^2 / subL / subR lie over X_low");
    constexpr int B_WORDS = WT::NSUB * SUB_STRIDE > HF_AUX_WORDS ? WT::NSUB * SUB_STRIDE : HF_AUX_WORDS;
    __shared__ float s_a[HFPS_WAVES][HF_XLOW_WORDS];      // HF: X_low           | PS: |s|^2, subL / subR
    __shared__ float s_b[HFPS_WAVES][B_WORDS];            // HF: sums (alpha)    | PS: sub-subband rows
    __shared__ float s_c[HFPS_WAVES][HFPS_C_WORDS];       // HF: header, channel | PS: band power / transient gain
    __shared__ HeaacPsFrame s_p[HFPS_WAVES];
    __shared__ float s_inb[HFPS_WAVES][WT::NLOW][44][2];
    __shared__ float s_Hs[HFPS_WAVES][6][WT::NH][WT::NPAR];
    __shared__ signed char s_idx[HFPS_WAVES][2][5][WT::NPAR];
    __shared__ float s_noise[1024];                       // sbr_noise_table, staged once per workgroup
    __shared__ float s_hyb[8 * 14 + 8];                   // 20-band hybrid filters: f20_0_8, g1_Q2
    __shared__ float s_dump[64];                          // where the L2 prefetches' LDS-DMA writes go (never read)
    wg_copy_f4(s_noise, g_tab + TB_NOISE, 1024);
    if (threadIdx.x < 112) s_hyb[threadIdx.x] = g_tab[TB_F20_0_8 + threadIdx.x];
    if (threadIdx.x < 8) s_hyb[112 + threadIdx.x] = g_tab[TB_G1_Q2 + threadIdx.x];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE;
    const HfWave H = hf_wave_view(s_a[wave], s_b[wave], s_c[wave]);
    WT W = { s_p[wave], s_inb[wave], s_a[wave], reinterpret_cast<float (*)[SUB_STRIDE]>(s_b[wave]),
             reinterpret_cast<float (*)[SUB_STRIDE]>(s_a[wave]),
             reinterpret_cast<float (*)[SUB_STRIDE]>(s_a[wave] + (WT::NSUB + 1) * SUB_STRIDE),
             reinterpret_cast<float (*)[33]>(s_c[wave]), s_Hs[wave], s_idx[wave][0], s_idx[wave][1],
             s_idx[wave][0], s_idx[wave][0], s_hyb, s_hyb + 112 };
    // Frames cost between ~0.8x and ~1.3x the mean (envelope counts, smoothing, patches): FrameFeed (k_common.h)
    // draws them from a queue.  The frame in work and the next one are
    // known; the next one's parameter records are touched into the caches two thirds into the PS pass of the
    // current frame.  Level 1 = the SBR and PS frame records (1.2 KB): k_hfps -6.8 %.  Level 2 adds W and the SBR
    // state (16 KB) for another 0.3 %, but those lines leave L2 again before they are used and are fetched twice
    // (measured: +14.5 KiB per frame of FETCH_SIZE; touched later they cost 3-5 %, profiles/r03_experiments.md E10).
    const unsigned sink = lds_addr(s_dump);
    FrameFeed<HFPS_QUEUE_CHUNK> feed;
    feed.init((unsigned long long)blockIdx.x * HFPS_WAVES + wave, (unsigned long long)gridDim.x * HFPS_WAVES, g_queue, lane);
    while (feed.cur < n_frames) {
        const unsigned long long f = feed.cur, f1 = feed.nxt;
        feed.request(lane);
        const unsigned long long rf = STRIDED ? f * rstride : f, rf1 = STRIDED ? f1 * rstride : f1;
        if constexpr (sizeof...(Hold) != 0) {
            if (__builtin_amdgcn_readfirstlane((int)hold_mask(hold...)[rf])) {
                feed.advance();
                continue;
            }
        }
        // slot of the PS loop at which the next frame's SBR and PS records (1.2 KB) are touched into L2
        constexpr int TOUCH_RECORDS_SLOT = 20;
        auto prefetch_next = [&](int n) {
            if (n == TOUCH_RECORDS_SLOT && f1 < n_frames) {
                l2_touch(&g_sbr[rf1], sizeof(HeaacSbrFrame), lane, sink);
                l2_touch(&g_ps[rf1], sizeof(HeaacPsFrame), lane, sink);
            }
        };
        const bool base = __builtin_amdgcn_readfirstlane(!ps_frame_is_general(&g_ps[rf]));
        // skip_fast is always 0.  It was 1 only behind the twelve-wave kernel of round 4 (profiles/r04_experiments.md E1,
        // removed), which took these frames first.  The argument and this branch are still here because without them the
        // SGPR spills of <false> / <true> / <true, hold> go from 78 / 80 / 83 to 81 / 77 / 77, and that has not been timed.
        if (skip_fast && base && __builtin_amdgcn_readfirstlane(hf_frame_is_fast(&g_sbr[rf], g_hdr, n_hdr))) {
            feed.advance();
            continue;
        }
        float *Xf = g_X + (f * 2) * HE_X_CHANNEL;
        v2f *Xf2 = reinterpret_cast<v2f *>(Xf);
        const float *st_in = g_state_in + f * state_words;
        float *st_out = g_state_out + f * state_words;
        v2f col[32];
        float (*inb)[44][2] = s_inb[wave];
        // the PS record and the hybrid filters' history are loaded here, beside the HF stage's
        // parameters, and stored to LDS in the same wait
        uint32_t preg[3];
        float hist_re = 0.0f, hist_im = 0.0f;
        {
            const uint32_t *ps_ = reinterpret_cast<const uint32_t *>(&g_ps[rf]);
#pragma unroll
            for (int r = 0; r < 3; r++) preg[r] = lane + 64 * r < (int)(sizeof(HeaacPsFrame) / 4) ? ps_[lane + 64 * r] : 0;
            if (lane < WT::NLOW * 6) {
                hist_re = st_in[off_ps + HEAAC_PS_INBUF + 2 * lane];
                hist_im = st_in[off_ps + HEAAC_PS_INBUF + 2 * lane + 1];
            }
        }
        hf_channel(H, s_noise, &g_sbr[rf], g_hdr, n_hdr, 0, g_W + f * 2048, st_in + off_sbr, st_out + off_sbr, lane,
                   [&](int i, float re, float im) {
                       if (i < 32) {
                           col[i] = v2f{re, im};
                       } else if (base) {
                           // look-ahead slots of the hybrid analysis (aacps.c:362-367)
                           if (lane < WT::NLOW) { inb[lane][6 + i][0] = re; inb[lane][6 + i][1] = im; }
                       } else {
                           Xf2[i * 64 + lane] = v2f{re, im};
                       }
                   },
                   [&]() {
                       uint32_t *pd = reinterpret_cast<uint32_t *>(&s_p[wave]);
#pragma unroll
                       for (int r = 0; r < 3; r++)
                           if (lane + 64 * r < (int)(sizeof(HeaacPsFrame) / 4)) pd[lane + 64 * r] = preg[r];
                       if (lane < WT::NLOW * 6) { inb[lane / 6][lane % 6][0] = hist_re; inb[lane / 6][lane % 6][1] = hist_im; }
                   });
        if (!base) {
#pragma unroll
            for (int i = 0; i < 32; i++) Xf2[i * 64 + lane] = col[i];
        } else {
            // ff_ps_apply(..., sbr->kx[1] + sbr->m[1]): the header is still in the HF stage's LDS
            const int top = __builtin_amdgcn_readfirstlane(H.h.kx + H.h.m);
            // sbr_x_gen's first i_Temp slots follow the previous frame's range (aacsbr.c:1419-1432): X is +0 above `top`
            // in EVERY slot if there are no such slots or that range ends inside this one
            const int t_old = H.c[0].t_env_num_env_old;
            const bool x_zero_above = __builtin_amdgcn_readfirstlane(
                2 * t_old - 32 <= 0 || (int)g_sbr[rf].kx_old + (int)g_sbr[rf].m_old <= ((top + 15) & ~15));
            ps_frame<false, true>(W, g_tab, &g_ps[rf], top, st_in + off_ps, st_out + off_ps, Xf, lane, wave, col,
                                  prefetch_next, g_xtop + 2 * f, x_zero_above);
        }
        feed.advance();
    }
    l2_touch_drain();
}

#define PS_WAVES_GEN 5

// The two HE-AACv2 launches of heaac_launch_he (k_he.hip) for position t of its streams: the records are read with a
// stride of T frames and the state by stream, from st_in; W / X are the hand-over units of position t.  One frame per
// stream without a hold mask runs the batch kernels (no record stride, no hold test).
// HF adjustment of the mono core channel fused with baseline Parametric Stereo
extern "C" int heaac_launch_hfps(const HeaacHeLaunch *a, size_t t, const float *st_in, const float *W, float *X)
{
    const HeaacCfgShape c = heaac_cfg_shape(a->cfg);
    const unsigned long long S = a->n_streams, T = a->T;
    with_strided_hold(T != 1, a->d_hold ? a->d_hold + t : nullptr, [&](auto st, auto... m) {
        k_hfps<st()><<<persistent_grid(S, HFPS_WAVES), HFPS_WAVES * WAVE, 0, a->s>>>(
            a->d_tab, a->d_sbr + t, a->d_hdr, a->n_hdr, a->d_ps + t, W, st_in, a->d_state_out, (int)c.words, c.off_sbr,
            c.off_ps, X, S, a->d_queue, a->d_xtop + 2 * t * S, 0, T, m...);
    });
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

// The frames k_hfps leaves (every layout but the baseline one)
extern "C" int heaac_launch_ps(const HeaacHeLaunch *a, size_t t, const float *st_in, float *X)
{
    const HeaacCfgShape c = heaac_cfg_shape(a->cfg);
    const unsigned long long S = a->n_streams, T = a->T;
    with_strided_hold(T != 1, a->d_hold ? a->d_hold + t : nullptr, [&](auto st, auto... m) {
        k_ps<true, PS_WAVES_GEN, st()><<<persistent_grid(S, PS_WAVES_GEN), PS_WAVES_GEN * WAVE, 0, a->s>>>(
            a->d_tab, a->d_ps + t, a->d_sbr + t, a->d_hdr, a->n_hdr, st_in, a->d_state_out, (int)c.words, c.off_ps, X, S, T,
            m...);
    });
    return hipGetLastError() == hipSuccess ? HEAAC_OK : HEAAC_ERR_HIP;
}

#ifdef HEAAC_STAMPS
// accumulated phase timeline of the fused kernel: out[0..31] cycles per phase, out[32] frames
extern "C" int heaac_debug_timeline(unsigned long long *out)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tl_acc), sizeof(g_tl_acc)) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out + 32, HIP_SYMBOL(g_tl_cnt), sizeof(g_tl_cnt)) == hipSuccess ? 0 : -1;
}
#endif
