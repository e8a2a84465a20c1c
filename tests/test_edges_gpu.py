"""GPU parity at the signal edges: the profiles of tests/edge_signals.py (silence, -0, sound then silence, subnormal
levels and fades, full scale and beyond, a tone, clicks; every SBR scalefactor 0..255, all harmonics, inverse
filtering at its extremes, the limiter's corners) against the oracle chained frame by frame.
tests/test_edge_reach.py shows, on the CPU, that these inputs take the branches they are for.

Bar: bit-exact f32 words (PCM and state) and identical int16, with one exception: where the oracle's word is a NaN,
any NaN matches.  x86 SSE makes the default NaN with the sign bit set (0xFFC00000), the GPU without it (0x7FC00000),
and later negations flip either.  On the env_sweep frames the first MI355X run showed only these two quiet NaNs on
both sides, in different places: HE-AACv1 PCM, for one, held 228 327 / 232 089 of them (0x7FC00000 / 0xFFC00000) on
the GPU against 337 284 / 123 132 in the oracle.  An inf must match an inf of the same sign (it is compared bit for
bit), int16 without exception, and a stream's chain must turn non-finite and finite again at the same frames as the
oracle's."""
import importlib

import numpy as np
import pytest

import edge_signals as E
from test_linear_scaling import STAGES, OracleStages, check_power_of_two_scaling, check_subnormal_range

pytestmark = pytest.mark.gpu

FMTS = ("PCM_F32", "PCM_S16", "PCM_S16_SSE2")


def _synth():
    return importlib.import_module("ffmpeg_heaac_amd.synth")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_words(got, ref, what):
    """f32 words bit for bit; a NaN of the reference is matched by any NaN"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ok = (_bits(got) == _bits(ref)) | (np.isnan(got) & np.isnan(ref))
    if not ok.all():
        i = np.argwhere(~ok)[:5].tolist()
        raise AssertionError("%s: %d words differ, first at %s (got %s, want %s)" % (
            what, int((~ok).sum()), i, got[tuple(np.argwhere(~ok)[0])], ref[tuple(np.argwhere(~ok)[0])]))


def _finite_rows(a):
    a = np.asarray(a)
    return np.isfinite(a.reshape(a.shape[0], -1).astype(np.float32)).all(axis=1)


def _check_pcm(pkg, fmt, got, ref, what):
    if fmt == pkg.PCM_F32:
        assert_words(got, ref, what)
        assert np.array_equal(_finite_rows(got), _finite_rows(ref)), what
    else:
        assert np.array_equal(got, ref), "%s: %d int16 samples differ" % (what, int((got != ref).sum()))


@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("fmtname", FMTS)
@pytest.mark.parametrize("cfgname,ps_mode", E.HE_CFGS)
@pytest.mark.parametrize("profile", E.PROFILES)
def test_he_edges(pkg, oracle, dev, profile, cfgname, ps_mode, fmtname, ds):
    """he_decode chained frame by frame, and he_decode_streams with T = 8 (the rings kept on chip across the call),
    both against the oracle chained frame by frame"""
    import torch
    synth = _synth()
    cfg, fmt = getattr(pkg, cfgname), getattr(pkg, fmtname)
    hdr = synth.default_headers(pkg, extra=True)
    n, T = E.streams(profile), E.min_steps(profile)
    frames = E.he_frames(pkg, synth, cfg, profile, n, T, E.SEED, hdr, ps_mode=ps_mode)
    state = np.zeros((n, pkg.STATE_WORDS[cfg]), np.float32)
    d_state = torch.from_numpy(state).cuda()
    d_hdr = pkg.to_device(hdr)
    ref_pcm = []
    for t, fr in enumerate(frames):
        ref, state = oracle.he_decode_batch(cfg, fr["coeffs"], fr["ics"], fr["sbr"], hdr, fr["ps"], state, fmt,
                                            downsampled=ds)
        ref_pcm.append(ref)
        pcm, d_state = dev.he_decode(cfg, torch.from_numpy(fr["coeffs"]).cuda(), pkg.to_device(fr["ics"]),
                                     pkg.to_device(fr["sbr"]), d_hdr,
                                     pkg.to_device(fr["ps"]) if fr["ps"] is not None else None, d_state,
                                     pcm_format=fmt, downsampled=ds)
        _check_pcm(pkg, fmt, pcm.cpu().numpy(), ref, "he_decode frame %d PCM" % t)
        assert_words(d_state.cpu().numpy(), state, "he_decode frame %d state" % t)
        assert np.array_equal(_finite_rows(d_state.cpu().numpy()), _finite_rows(state)), t
    # the same frames in one streams call: frame t of stream s at s * T + t
    stack = lambda k: np.ascontiguousarray(np.stack([f[k] for f in frames], axis=1).reshape(
        (n * T,) + frames[0][k].shape[1:]))
    ps = stack("ps") if frames[0]["ps"] is not None else None
    pcm, st = dev.he_decode_streams(cfg, torch.from_numpy(stack("coeffs")).cuda(), pkg.to_device(stack("ics")),
                                    pkg.to_device(stack("sbr")), d_hdr, pkg.to_device(ps) if ps is not None else None,
                                    torch.zeros((n, pkg.STATE_WORDS[cfg]), dtype=torch.float32, device="cuda"), T,
                                    pcm_format=fmt, downsampled=ds)
    torch.cuda.synchronize()
    got = pcm.cpu().numpy().reshape((n, T) + tuple(pcm.shape[1:]))
    for t in range(T):
        _check_pcm(pkg, fmt, got[:, t], ref_pcm[t], "streams frame %d PCM" % t)
    assert_words(st.cpu().numpy(), state, "streams final state")


@pytest.mark.parametrize("fmtname", FMTS[:2])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", E.CORE_PROFILES)
def test_lc_edges(pkg, oracle, dev, profile, channels, fmtname):
    import torch
    fmt = getattr(pkg, fmtname)
    n = E.STREAMS
    state = np.zeros((n, channels * 512), np.float32)
    d_state = torch.from_numpy(state).cuda()
    for t, (coeffs, ics) in enumerate(E.lc_frames(_synth(), profile, n, E.min_steps(profile), E.SEED, channels)):
        ref, state = oracle.lc_decode_batch(channels, coeffs, ics, state, fmt)
        pcm, d_state = dev.lc_decode(channels, torch.from_numpy(coeffs).cuda(), pkg.to_device(ics), d_state,
                                     pcm_format=fmt)
        _check_pcm(pkg, fmt, pcm.cpu().numpy(), ref, "lc frame %d PCM" % t)
        assert_words(d_state.cpu().numpy(), state, "lc frame %d state" % t)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", ["fade", "sound_then_silence"])
def test_main_prediction_edges(pkg, oracle, dev, profile, channels):
    """AAC-Main prediction (PNS ahead of it, M/S, intensity and TNS after): the predictor state goes subnormal under
    the fade, and var <= 1 (k = 0) after every reset (test_edge_reach)"""
    import torch
    synth = _synth()
    n = E.STREAMS * 4
    rng = np.random.default_rng(E.SEED)
    pred = np.zeros((n, channels, pkg.MAX_PREDICTORS), pkg.PRED_STATE_DT)
    pred["var0"] = 1.0
    pred["var1"] = 1.0
    pred = pred.view(np.float32).reshape(n, channels, pkg.MAX_PREDICTORS, 6)
    rs = np.full(n, 0x1f2e3d4c, np.int32)
    d_rs, d_pred = torch.from_numpy(rs.copy()).cuda(), torch.from_numpy(pred.copy()).cuda()
    for step in range(E.min_steps(profile)):
        tools = synth.tools_frames(rng, pkg, n, channels)
        coeffs = E.tools_coeffs(profile, rng, n, channels, step)
        ref, rs, pred = oracle.spectral_tools_batch(channels, coeffs, tools, rs, pred)
        d = torch.from_numpy(coeffs).cuda()
        dev.spectral_tools(channels, d, pkg.to_device(tools), rng=d_rs, pred=d_pred)
        assert_words(d.cpu().numpy(), ref, "step %d coefficients" % step)
        assert np.array_equal(d_rs.cpu().numpy(), rs), step
        assert_words(d_pred.cpu().numpy(), pred, "step %d predictor state" % step)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", ["subnormal", "loud", "neg_zero", "fade"])
def test_spectral_tools_edges(pkg, oracle, dev, profile, channels):
    """M/S, intensity and TNS (all on in tools_frames) on subnormal, loud and -0 spectra"""
    import torch
    synth = _synth()
    n = E.STREAMS * 8
    rng = np.random.default_rng(E.SEED + 1)
    for step in range(3):
        tools = synth.tools_frames(rng, pkg, n, channels)
        coeffs = E.tools_coeffs(profile, rng, n, channels, step)
        ref = oracle.spectral_tools_batch(channels, coeffs, tools)
        d = torch.from_numpy(coeffs).cuda()
        dev.spectral_tools(channels, d, pkg.to_device(tools))
        assert_words(d.cpu().numpy(), ref, "step %d" % step)


class DeviceStages:
    """the HIP stages with OracleStages' interface"""

    def __init__(self, dev):
        self.d = dev

    @staticmethod
    def _t(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()

    def imdct(self, which, x):
        return (self.d.imdct_half(which, self._t(x)).cpu().numpy(),)

    def analysis(self, x, xh):
        W, xo = self.d.qmf_analysis(self._t(x), self._t(xh), scale=1.0)
        return W.cpu().numpy(), xo.cpu().numpy()

    def synthesis(self, X, v):
        out, vo = self.d.qmf_synthesis(self._t(X), self._t(v), scale=1.0, bias=0.0)
        return out.cpu().numpy(), vo.cpu().numpy()

    def synthesis_ds(self, X, v):
        out, vo = self.d.qmf_synthesis_ds(self._t(X), self._t(v), scale=1.0, bias=0.0)
        return out.cpu().numpy(), vo.cpu().numpy()


@pytest.mark.parametrize("name", STAGES)
def test_stage_power_of_two_scaling(dev, name):
    check_power_of_two_scaling(DeviceStages(dev), name)


@pytest.mark.parametrize("name", STAGES)
def test_stage_subnormal_range(oracle, dev, name):
    check_subnormal_range(DeviceStages(dev), OracleStages(oracle), name)


@pytest.mark.parametrize("level", ["subnormal", "loud"])
@pytest.mark.parametrize("name", STAGES)
def test_stage_edges_match_oracle(oracle, dev, name, level):
    """each stage bit for bit against the oracle at the campaign's subnormal scales and at the loud levels (the
    analysis and synthesis with their codec scales, 32768 and 2^-15 with the 385 bias)"""
    import test_linear_scaling as L
    args = L.inputs(name, 6, 11)
    g = ([2.0 ** -106, 2.0 ** -126, 2.0 ** -146] if level == "subnormal" else [E.LOUD[1] * 16, E.LOUD[1] * 1024])
    for k, gain in enumerate(g):
        a = tuple((np.asarray(x, np.float64) * gain).astype(np.float32) for x in args)
        if name.startswith("imdct"):
            got, ref = DeviceStages(dev).imdct(int(name[-1]), *a), OracleStages(oracle).imdct(int(name[-1]), *a)
        elif name == "analysis":
            import torch
            W, xo = dev.qmf_analysis(torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda())
            got = (W.cpu().numpy(), xo.cpu().numpy())
            r = [oracle.qmf_analysis(a[0][i], a[1][i]) for i in range(a[0].shape[0])]
            ref = (np.stack([x for x, _ in r]), np.stack([y for _, y in r]))
        else:
            import torch
            f = dev.qmf_synthesis if name == "synthesis" else dev.qmf_synthesis_ds
            of = oracle.qmf_synthesis if name == "synthesis" else oracle.qmf_synthesis_ds
            out, vo = f(torch.from_numpy(a[0]).cuda(), torch.from_numpy(a[1]).cuda())
            got = (out.cpu().numpy(), vo.cpu().numpy())
            r = [of(a[0][i], a[1][i]) for i in range(a[0].shape[0])]
            ref = (np.stack([x for x, _ in r]), np.stack([y for _, y in r]))
        for x, y in zip(got, ref):
            assert_words(x, y, "%s x %g" % (name, gain))
