"""The edge-signal campaign reaches the edges (CPU, oracle only): every profile of tests/edge_signals.py, run through
the oracle exactly as tests/test_edges_gpu.py runs it, takes the branches it is meant for (oracle branch counters),
so that the GPU parity test on these inputs says something about those branches."""
import importlib

import numpy as np
import pytest

import edge_signals as E


def _synth():
    return importlib.import_module("ffmpeg_heaac_amd.synth")


# profile -> branches it must take somewhere in its runs (oracle.h OR_BR_*)
EXPECT = {
    "silence": ("dk_zero", "phi100_zero", "gain_max_1e5", "gain_boost_cap"),
    "neg_zero": ("dk_zero", "phi100_zero", "gain_max_1e5"),
    "sound_then_silence": ("dk_zero", "phi100_zero", "gain_clamp", "q_m_clamp"),
    "subnormal": ("dk_zero", "phi100_zero"),
    "fade": ("dk_zero", "gain_clamp", "q_m_clamp"),
    "full_scale": ("gain_clamp", "s16_high", "s16_low"),
    "loud": ("gain_clamp", "s16_high", "s16_low"),
    "tone": ("gain_max_1e5", "gain_clamp", "gain_boost_cap"),
    "impulse": ("alpha_reset", "dk_zero", "s16_high", "s16_low"),
    "env_sweep": ("exp2_inf", "exp2_subnormal", "s16_sse2_high", "s16_sse2_low"),
    "noise_sweep": ("exp2_subnormal",),
    "harmonic_invf": ("gain_clamp", "gain_boost_cap"),
    "loud_env_silence": ("gain_max_1e5", "gain_clamp", "q_m_clamp", "gain_boost_cap"),
    "min_env_loud": ("gain_clamp", "gain_boost_cap", "s16_high", "s16_low"),
}


def _subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < np.finfo(np.float32).tiny)


def _run(pkg, oracle, profile):
    """every configuration, PCM format and bank of the GPU campaign; returns (counts, facts)"""
    synth = _synth()
    hdr = synth.default_headers(pkg, extra=True)
    oracle.branch_reset()
    facts = dict(nonfinite=0, finite_after=0, subnormal_state=0, frames=0)
    n = E.streams(profile)
    for cfgname, ps_mode in E.HE_CFGS:
        cfg = getattr(pkg, cfgname)
        frames = E.he_frames(pkg, synth, cfg, profile, n, E.min_steps(profile), E.SEED, hdr, ps_mode=ps_mode)
        for fmt in (oracle.PCM_F32, oracle.PCM_S16, oracle.PCM_S16_SSE2):
            for ds in (False, True):
                state = np.zeros((n, pkg.STATE_WORDS[cfg]), np.float32)
                bad = np.zeros(n, bool)
                for fr in frames:
                    pcm, state = oracle.he_decode_batch(cfg, fr["coeffs"], fr["ics"], fr["sbr"], hdr, fr["ps"], state,
                                                        fmt, downsampled=ds)
                    facts["frames"] += n
                    facts["subnormal_state"] += int(_subnormal(state).any(axis=1).sum())
                    if fmt == oracle.PCM_F32:
                        nf = ~np.isfinite(pcm).all(axis=(1, 2))
                        facts["nonfinite"] += int(nf.sum())
                        facts["finite_after"] += int((bad & ~nf).sum())
                        bad |= nf
    return oracle.branch_counts(), facts


@pytest.mark.parametrize("profile", E.PROFILES)
def test_profile_reaches_its_branches(pkg, oracle, profile):
    counts, facts = _run(pkg, oracle, profile)
    missing = [b for b in EXPECT[profile] if not counts[b]]
    assert not missing, "%s takes none of %s (counts %s)" % (profile, missing, counts)
    if profile in ("subnormal", "fade", "sound_then_silence"):
        # IMDCT output, QMF rings and delay lines cross the subnormal range: a flushing build changes state words
        assert facts["subnormal_state"] > 0
    if profile == "env_sweep":
        # envelopes that dequantise to inf make non-finite frames, and the chains come back to finite output
        assert facts["nonfinite"] > 0 and facts["finite_after"] > 0, facts
    elif profile not in ("loud_env_silence",):
        # the X^2 bound of edge_signals: every other profile, the loud ones included, stays finite
        assert facts["nonfinite"] == 0, facts


def test_all_branches_reached(pkg, oracle):
    """the union over the HE profiles leaves no HE counter at zero (the predictor's are the tools test's)"""
    total = {}
    for profile in E.PROFILES:
        for k, v in _run(pkg, oracle, profile)[0].items():
            total[k] = total.get(k, 0) + v
    zero = [k for k, v in total.items() if not v and not k.startswith("pred_")]
    assert not zero, zero


def test_env_sweep_covers_every_value(pkg):
    """every env_facs_q and noise_facs_q value 0..255 is read by some frame, at amp_res 0 and 1, uncoupled and
    coupled (channel 0 and the balance channel 1); noise floors have no amp_res"""
    synth = _synth()
    hdr = synth.default_headers(pkg, extra=True)
    seen = {}
    n = E.streams("env_sweep")
    for profile, field in (("env_sweep", "env_facs_q"), ("noise_sweep", "noise_facs_q")):
        for cfgname, ps_mode in E.HE_CFGS:
            cfg = getattr(pkg, cfgname)
            for fr in E.he_frames(pkg, synth, cfg, profile, n, E.min_steps(profile), E.SEED, hdr,
                                  ps_mode=ps_mode):
                for s in range(n):
                    f = fr["sbr"][s]
                    if not f["start"]:
                        continue
                    h = hdr[int(f["hdr"])]
                    for c in range(2 if cfg == pkg.CFG_HEV1 else 1):
                        ch = f["ch"][c]
                        amp = int(f["ch"][0]["bs_amp_res"])
                        cp = int(f["bs_coupling"])
                        key = (field, amp if field == "env_facs_q" else 0, cp, c if cp else 0)
                        if field == "env_facs_q":
                            vals = [ch[field][e, :int(h["n"][int(ch["bs_freq_res"][e + 1])])]
                                    for e in range(int(ch["bs_num_env"]))]
                        else:
                            vals = [ch[field][e, :int(h["n_q"])] for e in range(int(ch["bs_num_noise"]))]
                        seen.setdefault(key, set()).update(int(v) for a in vals for v in a)
    classes = ((0, 0), (1, 0), (1, 1))          # (coupled, channel): uncoupled channels share one class
    for key in [("env_facs_q", a, cp, c) for a in (0, 1) for cp, c in classes] + \
               [("noise_facs_q", 0, cp, c) for cp, c in classes]:
        missing = sorted(set(range(256)) - seen.get(key, set()))
        assert not missing, "%s: %d values never read, first %s" % (key, len(missing), missing[:8])


@pytest.mark.parametrize("profile", ["fade", "sound_then_silence"])
def test_predictor_reaches_its_branches(pkg, oracle, profile):
    """AAC-Main prediction under a fade and under silence: var <= 1 (k = 0), and under the fade subnormal predictor
    state"""
    synth = _synth()
    n, channels = E.STREAMS * 4, 2
    rng = np.random.default_rng(E.SEED)
    pred = np.zeros((n, channels, pkg.MAX_PREDICTORS), pkg.PRED_STATE_DT)
    pred["var0"] = 1.0
    pred["var1"] = 1.0
    pred = pred.view(np.float32).reshape(n, channels, pkg.MAX_PREDICTORS, 6)
    rs = np.full(n, 0x1f2e3d4c, np.int32)
    oracle.branch_reset()
    for step in range(E.min_steps(profile)):
        tools = synth.tools_frames(rng, pkg, n, channels)
        coeffs = E.tools_coeffs(profile, rng, n, channels, step)
        _, rs, pred = oracle.spectral_tools_batch(channels, coeffs, tools, rs, pred)
    counts = oracle.branch_counts()
    assert counts["pred_var_le1"], counts
    if profile == "fade":
        # (under silence the state only decays by 29/32 a frame: it stays normal)
        assert counts["pred_subnormal"], counts


def _exp2_half(twice):
    """csrc/k_hf.h exp2_half, restated on the host (float32 arithmetic)"""
    def normal(t):
        e = t >> 1
        mant = 0x3FB504F3 if t & 1 else 0x3F800000
        return np.array([(mant + (e << 23)) & 0xFFFFFFFF], np.uint32).view(np.float32)[0]
    if twice > 255:
        return np.float32(np.inf)
    if twice < -252:
        return np.float32(0.0) if twice < -400 else np.float32(normal(twice + 256) * np.float32(2.0 ** -128))
    return normal(twice)


def test_exp2_half_equals_libm_on_every_record_value():
    """Every exp2f argument sbr_dequant forms from uint8 records (aacsbr.c:1099-1125; 2x the argument as the kernels
    pass it, k_hf.h deq_env / deq_noise): the GPU's exp2_half equals libm bit for bit, the inf above twice = 255 and
    the subnormal side included.  The one place exp2_half rounds twice (an odd argument below -126) is not reachable:
    odd arguments only come from amp_res 0 envelopes, q + 12 >= 12 and the coupled balance 24 - q >= -231."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.exp2f.restype = ctypes.c_float
    libm.exp2f.argtypes = [ctypes.c_float]
    q = range(256)
    twice = set()
    for v in q:
        twice |= {2 * v + 12, v + 12,                    # envelope, amp_res 1 / 0
                  2 * v + 14, v + 14,                    # coupled envelope, channel 0
                  2 * (12 - v), 24 - v,                  # coupled balance, channel 1
                  2 * (7 - v), 2 * (12 - v), 2 * (6 - v)}   # noise floors: coupled 0 / 1, uncoupled
    assert not [t for t in twice if t & 1 and t < -252]
    subnormal = 0
    for t in sorted(twice):
        ref = np.float32(libm.exp2f(ctypes.c_float(t / 2.0)))
        got = _exp2_half(t)
        assert np.array_equal(np.array([got]).view(np.uint32), np.array([ref]).view(np.uint32)), (t, got, ref)
        subnormal += 0 < ref < np.finfo(np.float32).tiny
    assert subnormal >= 20 and max(twice) > 255
