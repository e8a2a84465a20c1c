"""Edge-signal profiles for the parity campaign (tests/test_edge_reach.py, tests/test_edges_gpu.py).

Host logic only (numpy).  Every generator here takes the frames of synth.he_stream / lc_stream / tools_frames as they
are and rewrites only values: the core spectrum, or the SBR scalefactors and the per-band flags.  The structure (window
sequences, SBR grids and borders, PS parameters) stays as the synth generators make it, and the synth generators and
their RNG draws are not touched (bench.py draws its inputs from them).

Levels.  synth._coeffs draws uniform noise at +-NORMAL = 4096 * |sf_scale| = 2^-13 per line; the IMDCT output of that
peaks near 0.006 of full scale (1.0 = 32768 in int16).  FULL = 2^-6 (NORMAL * 2^7) puts a noise frame's peak near
full scale.

Bound on the X^2 sums (the loud profiles).  With lines of at most A: |IMDCT output| <= 2 * 651.9 * A (L1 norm of an
IMDCT row, two overlapping halves, windows <= 1); the analysis bank scales by 32768 and its 320-tap prototype
(qmf_ds) has L1 norm 54.19 with the folding, so |W| <= 2 * 54.19 * 32768 * 2 * 651.9 * A; an autocorrelation sum over
40 slots of |X|^2 is at most 80 |W|^2, i.e. <= 2^44.54 * (A / NORMAL)^2, and e_curr (X_high <= 9 |X_low| after the
|alpha|^2 < 16 reset) is at most 2^45.56 * (A / NORMAL)^2.  dk multiplies two such sums: it stays finite while each
sum is <= 2^63, i.e. A <= 2^-3.77.  LOUD = (4 FULL, 64 FULL) = (2^-4, 2^0): the first keeps even the worst-case bound
finite (sums <= 2^62.5); at the second the worst-case bound is 2^70.5, but for this noise (peaks ~26x under the
bound, energies ~2^9.4 under) the oracle's PCM stays finite, which test_edge_reach asserts.
"""
import numpy as np

SF_SCALE = 1.0 / (1024.0 * 32768.0)
NORMAL = 4096 * SF_SCALE                  # 2^-13, synth._coeffs
FULL = NORMAL * 2.0 ** 7                  # 2^-6: a noise frame peaks near full scale
LOUD = (4.0, 64.0)                        # times FULL (see the bound above)
SUBNORMAL_SCALES = (2.0 ** -100, 2.0 ** -120, 2.0 ** -140)   # times FULL: lines at 2^-106, 2^-126, 2^-146
FADE_OCTAVES = 8                          # per frame: x 2^-8
FADE_OFFSETS = (0, 64, 128)               # octaves below FULL at the first frame, by stream: 0 .. -184 in 8 frames

# sound_then_silence: frames of the normal profile, then +0.  DRAIN_FRAMES silent frames empty every ring: the
# overlap buffer (1024 samples at the core rate), the analysis history (288), the W / X_low tail (8 QMF slots of 32
# samples), the PS delay lines (at most 14 slots) and the smoothing tails (4 slots), the synthesis ring (1152 / 1280
# floats = 9 / 10 slots; 576 in the downsampled bank): together < 2.5 frames of 1024; 4 leave margin.
SOUND_FRAMES = 3
DRAIN_FRAMES = 4

TONE_LINE = 37                            # one MDCT line (and its neighbour for the pair), long windows

CORE_PROFILES = ("silence", "neg_zero", "sound_then_silence", "subnormal", "fade", "full_scale", "loud", "tone",
                 "impulse")
SBR_PROFILES = ("env_sweep", "noise_sweep", "harmonic_invf", "loud_env_silence", "min_env_loud")
PROFILES = CORE_PROFILES + SBR_PROFILES
# the core profile that goes with each SBR profile (the others keep the normal spectrum)
SBR_CORE = {"loud_env_silence": "silence", "min_env_loud": "loud"}

EIGHT_SHORT_SEQUENCE = 2

# the campaign's HE configurations (cfg name, PS mode) and sizes: tests/test_edge_reach.py runs the oracle on exactly
# what tests/test_edges_gpu.py runs on the GPU
HE_CFGS = (("CFG_HEV1", "20"), ("CFG_HEV1_MONO", "20"), ("CFG_HEV2", "20"), ("CFG_HEV2", "mix"))
STREAMS = 8
SEED = 2024


def min_steps(profile):
    """frames a chain needs for the profile to do what it is for"""
    return SOUND_FRAMES + DRAIN_FRAMES + 1 if profile == "sound_then_silence" else 8


def streams(profile):
    """streams of a run: the sweeps need enough coupled amp_res-0 envelopes to read all 256 values"""
    return 4 * STREAMS if profile in ("env_sweep", "noise_sweep") else STREAMS


def core(profile, coeffs, ics, step):
    """Rewrite one step's core spectrum [n][ch][1024] (float32, the synth's normal noise) for `profile`; ics [n][ch]
    gives the window sequence (EIGHT_SHORT frames hold eight 128-line windows).  Returns a new array."""
    c = np.array(coeffs, np.float32, copy=True)
    n = c.shape[0]
    s = np.arange(n)
    if profile in ("normal",) + SBR_PROFILES and profile not in SBR_CORE:
        return c
    profile = SBR_CORE.get(profile, profile)
    if profile == "silence":
        return np.zeros_like(c)
    if profile == "neg_zero":
        return np.full_like(c, -0.0)
    if profile == "sound_then_silence":
        return c if step < SOUND_FRAMES else np.zeros_like(c)
    c64 = c.astype(np.float64)
    if profile == "subnormal":
        g = np.array(SUBNORMAL_SCALES)[s % 3] * (FULL / NORMAL)
        return (c64 * g[:, None, None]).astype(np.float32)
    if profile == "fade":
        octaves = np.array(FADE_OFFSETS)[s % 3] + FADE_OCTAVES * step
        g = np.exp2(-octaves.astype(np.float64)) * (FULL / NORMAL)
        return (c64 * g[:, None, None]).astype(np.float32)
    if profile == "full_scale":
        return (c64 * (FULL / NORMAL)).astype(np.float32)
    if profile == "loud":
        g = np.array(LOUD)[s % 2] * (FULL / NORMAL)
        return (c64 * g[:, None, None]).astype(np.float32)
    short = np.asarray(ics["window_sequence"])[..., 0] == EIGHT_SHORT_SEQUENCE      # [n][ch]
    out = np.zeros_like(c)
    if profile == "tone":
        # one line (odd streams: a line pair) at a steady level; the phase walks by a quarter turn per frame, so
        # every QMF band the line leaks into sees one complex exponential: rank-1 covariances
        ph = 0.5 * np.pi * step + 0.3 * s
        amp = 0.25
        for w in range(8):
            k = w * 128 + TONE_LINE // 8
            out[:, :, k] = np.where(short, amp * np.cos(ph)[:, None] / 4, 0)
            out[:, :, k + 1] = np.where(short & (s % 2 == 1)[:, None], amp * np.sin(ph)[:, None] / 4, 0)
        out[:, :, TONE_LINE] = np.where(short, 0, amp * np.cos(ph)[:, None])
        out[:, :, TONE_LINE + 1] = np.where(short | (s % 2 == 0)[:, None], 0, amp * np.sin(ph)[:, None])
        return out
    if profile == "impulse":
        # two clicks per stream, in frames 1 + s % 3 and 5 + s % 3, with silence around them: the MDCT of a unit
        # impulse at sample n0 of the 2048-sample block (n0 walks with stream and frame), lines
        # A cos(pi / 1024 (n0 + 1/2 + 512)(k + 1/2));
        # EIGHT_SHORT frames take a flat spectrum.  An onset near the end of the X_low window makes the one-tap
        # predictor of a band the ratio of two slots of the prototype's rising edge: the |alpha|^2 >= 16 reset
        hit = (step == 1 + s % 3) | (step == 5 + s % 3)
        n0 = (s * 389 + step * 211 + 1100) % 2048
        k = np.arange(1024)
        lines = 0.25 * np.cos(np.pi / 1024 * (n0[:, None] + 0.5 + 512) * (k[None, :] + 0.5))
        out[:] = np.where(short[:, :, None], FULL * 0.25, lines[:, None, :]).astype(np.float32)
        out[~hit] = 0
        return out
    raise KeyError(profile)


# ---------------------------------------------------------------------------
# SBR records
# ---------------------------------------------------------------------------
def sbr(profile, sbr_fr, index, step, hdr, sweep):
    """Rewrite one step's SBR frames [n] in place for `profile`.  `index` [n] numbers the (stream, frame) pairs of the
    whole run; `step` is the frame's place in its chain; `hdr` the header table; `sweep` a dict that carries the
    sweeps' positions from call to call (one per run)."""
    for s in range(sbr_fr.shape[0]):
        fr = sbr_fr[s]
        if not fr["start"]:
            continue
        f = int(index[s])
        h = hdr[int(fr["hdr"])]
        coupled = int(fr["bs_coupling"])
        for c in range(2):
            ch = fr["ch"][c]
            if not ch["bs_num_env"]:
                continue
            bal = bool(coupled and c == 1)
            if profile in ("env_sweep", "noise_sweep"):
                # every value 0..255: each envelope (noise floor) reads the next values of its class's sweep, as many
                # as it has bands, so a class covers 0..255 once it has read 256 values.  Classes: amp_res (which
                # doubles the exponent), coupling, and for coupled pairs the channel (channel 1: the balance, swept the
                # other way, 255 .. 0)
                env = profile == "env_sweep"
                field = "env_facs_q" if env else "noise_facs_q"
                key = (field, int(fr["ch"][0]["bs_amp_res"]) if env else 0, coupled, c if coupled else 0)
                pos = sweep.get(key, 0)
                for e in range(int(ch["bs_num_env"]) if env else int(ch["bs_num_noise"])):
                    nb = int(h["n"][int(ch["bs_freq_res"][e + 1])]) if env else int(h["n_q"])
                    v = (pos + np.arange(ch[field].shape[1])) % 256
                    ch[field][e] = (255 - v) if bal else v
                    pos += nb
                sweep[key] = pos
            elif profile == "harmonic_invf":
                # a sinusoid on every band, inverse filtering at its extremes (3 / 0, alternating per frame: the
                # 0 <-> 3 transitions); bs_invf_mode[1] is the previous frame's [0] as the parser leaves it
                ch["bs_add_harmonic_flag"] = 1
                ch["bs_add_harmonic"][:] = 1
                ch["bs_invf_mode"][0] = 3 if (f % 2) else 0
                if step:
                    ch["bs_invf_mode"][1] = 0 if (f % 2) else 3
            elif profile == "loud_env_silence":
                # the loudest finite envelope over a silent core: e_curr = 0, the 1e5 clamp of gain_max
                amp = int(ch["bs_amp_res"])
                if bal:
                    ch["env_facs_q"][:] = 12 if amp else 24           # centre balance
                else:
                    ch["env_facs_q"][:] = (100 - f % 20) if amp else (200 - f % 40)
                ch["noise_facs_q"][:] = 12 if bal else f % 4
            elif profile == "min_env_loud":
                # the quietest envelope over a loud core: gains far below 1, the gain_boost cap
                ch["env_facs_q"][:] = 12 if bal else 0
                if not bal:
                    ch["noise_facs_q"][:] = 30 + f % 8
            else:
                raise KeyError(profile)


def he_frames(pkg, synth, cfg, profile, n, steps, seed, hdr, ps_mode="20"):
    """synth.he_stream frames (every header of `hdr` in turn, half the HE-AACv1 pairs coupled) rewritten for
    `profile`: a list of {coeffs, ics, sbr, ps} per step."""
    rng = np.random.default_rng(seed)
    frames = list(synth.he_stream(rng, cfg, n, steps, hdr, ps_mode=ps_mode, hdr_choice=np.arange(n) % len(hdr),
                                  coupling=0.5 if cfg == pkg.CFG_HEV1 else 0.0))
    sweep = {}
    for t, fr in enumerate(frames):
        fr["coeffs"] = core(profile, fr["coeffs"], fr["ics"], t)
        if profile in SBR_PROFILES:
            sbr(profile, fr["sbr"], np.arange(n) * steps + t, t, hdr, sweep)
    return frames


def lc_frames(synth, profile, n, steps, seed, channels):
    """synth.lc_stream steps rewritten for a core profile: a list of (coeffs, ics)."""
    rng = np.random.default_rng(seed)
    return [(core(profile, c, ics, t), ics) for t, (c, ics) in enumerate(synth.lc_stream(rng, n, steps, channels))]


def tools_coeffs(profile, rng, n, channels, step):
    """Spectra for the spectral tools at a core profile's level (standard normal, the tools tests' shape)."""
    base = (rng.standard_normal((n, channels, 1024)) * NORMAL).astype(np.float32)
    ics = np.zeros((n, channels), [("window_sequence", "u1", (2,))])
    return core(profile, base, ics, step)
