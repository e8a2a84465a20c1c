"""The hold masks of the streams calls (heaac_lc_decode_streams_ex, heaac_he_decode_streams_ex,
heaac_spectral_tools_streams_ex) on the GPU, bit for bit against code that knows no mask: T chained batch calls over
all S streams, where after step t the held streams' state rows (tools: generator and predictor rows) are put back to
what they were before the step and their PCM rows are zeroed.

In every call with a mask the held frames' per-frame records are overwritten with 0xFF bytes first (the reference runs
on the clean records): a held frame's records are not read, so the result may not change.  The synthetic records are
finite, so every frame of every stream is compared."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TS = [1, 2, 5, 8]
MASKS = ("none", "all", "first", "last", "middle", "random")


def _synth():
    return importlib.import_module("ffmpeg_heaac_amd.synth")


def _mask(kind, S, T, seed):
    """[S][T] uint8.  The partial masks leave some streams alone and hold different frames in neighbouring streams, so
    that the two half-waves of a mono pair differ."""
    m = np.zeros((S, T), np.uint8)
    s = np.arange(S)
    if kind == "all":
        m[:] = 1
    elif kind == "first":
        m[s % 3 != 1, 0] = 1
    elif kind == "last":
        m[s % 3 != 0, T - 1] = 1
    elif kind == "middle":
        lo = T // 3
        m[s % 2 == 0, lo:max(lo + 1, (2 * T) // 3)] = 1
        if T == 1:
            m[:] = (s % 2 == 0)[:, None]
    elif kind == "random":
        m[:] = np.random.default_rng(seed).random((S, T)) < 0.25
        m[0, 0] = 1                                   # (never empty)
        if T > 1:
            m[0, 1] = 0
    if kind not in ("none", "all"):
        assert m.any() and not m.all(), kind
        if T > 1:
            assert ((m.sum(axis=1) > 0) & (m.sum(axis=1) < T)).any(), "no stream has both a held and an unheld frame"
    return m


def _flat(a):
    a = np.ascontiguousarray(a)
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


def _poisoned(a, mask):
    """[S][T] records flattened to the streams layout, the held frames' bytes all 0xFF"""
    if a is None:
        return None
    f = _flat(a).copy()
    f.view(np.uint8).reshape(f.shape[0], -1)[mask.reshape(-1) != 0] = 0xFF
    return f


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, ref, what):
    import torch
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    g, r = got.contiguous().view(torch.uint8), ref.contiguous().view(torch.uint8)
    bad = g != r
    assert not bool(bad.any()), "%s: %d bytes differ, first at %s" % (what, int(bad.sum()),
                                                                       torch.nonzero(bad.reshape(-1))[:3].reshape(-1).tolist())


# ---------------------------------------------------------------------------------------------------------------
# AAC-LC
# ---------------------------------------------------------------------------------------------------------------
def _lc_inputs(pkg, dev, channels, S, T, seed):
    """[S][T] coefficients and ICS, and a state that one decoded frame has left (not all zeros)"""
    import torch
    steps = list(_synth().lc_stream(np.random.default_rng(seed), S, T + 1, channels))
    coeffs = np.stack([c for c, _ in steps], axis=1)
    ics = np.stack([i for _, i in steps], axis=1)
    _, state = dev.lc_decode(channels, _t(coeffs[:, 0]), pkg.to_device(np.ascontiguousarray(ics[:, 0])),
                             torch.zeros((S, channels * 512), device="cuda"))
    return coeffs[:, 1:], ics[:, 1:], state


def _lc_reference(pkg, dev, channels, coeffs, ics, state, mask, fmt):
    import torch
    S, T = mask.shape
    held = torch.from_numpy(mask != 0).cuda()
    state = state.clone()
    pcms = []
    for t in range(T):
        before = state.clone()
        pcm, state = dev.lc_decode(channels, _t(coeffs[:, t]), pkg.to_device(np.ascontiguousarray(ics[:, t])), before,
                                   pcm_format=fmt)
        state[held[:, t]] = before[held[:, t]]
        pcm[held[:, t]] = 0
        pcms.append(pcm)
    return torch.stack(pcms, dim=1), state


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("fmtname", ["PCM_F32", "PCM_S16", "PCM_S16_SSE2"])
@pytest.mark.parametrize("channels", [1, 2])
def test_lc_streams_hold(pkg, dev, channels, fmtname, T):
    import torch
    fmt = getattr(pkg, fmtname)
    S = 13 if channels == 1 else 6               # mono: odd, the last wave's second half is the masked tail
    coeffs, ics, state = _lc_inputs(pkg, dev, channels, S, T, 300 + T)
    for kind in MASKS:
        mask = _mask(kind, S, T, 17 * T + channels)
        ref_pcm, ref_state = _lc_reference(pkg, dev, channels, coeffs, ics, state, mask, fmt)
        st_out = torch.full_like(state, 7.0)
        pcm, st = dev.lc_decode_streams(channels, _t(_poisoned(coeffs, mask)), pkg.to_device(_poisoned(ics, mask)),
                                        state, T, state_out=st_out, pcm_format=fmt, hold=_t(_flat(mask)))
        torch.cuda.synchronize()
        _same(pcm.reshape(ref_pcm.shape), ref_pcm, "%s PCM" % kind)
        _same(st, ref_state, "%s state" % kind)
        if kind == "all":
            _same(st, state, "all held: state_out is state_in")
            assert not bool(pcm.view(torch.uint8).any()), "all held: PCM is zero bytes"
        # in place
        st_io = state.clone()
        pcm, _ = dev.lc_decode_streams(channels, _t(_poisoned(coeffs, mask)), pkg.to_device(_poisoned(ics, mask)),
                                       st_io, T, state_out=st_io, pcm_format=fmt, hold=_t(_flat(mask)))
        _same(pcm.reshape(ref_pcm.shape), ref_pcm, "%s PCM, in place" % kind)
        _same(st_io, ref_state, "%s state, in place" % kind)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("channels", [1, 2])
def test_lc_streams_no_mask_and_zero_mask_are_the_plain_call(pkg, dev, channels, T):
    import torch
    S = 9
    coeffs, ics, state = _lc_inputs(pkg, dev, channels, S, T, 350 + T)
    d_c, d_i = _t(_flat(coeffs)), pkg.to_device(_flat(ics))
    for fmt in (pkg.PCM_F32, pkg.PCM_S16):
        plain = dev.lc_decode_streams(channels, d_c, d_i, state, T, pcm_format=fmt)
        none = dev.lc_decode_streams(channels, d_c, d_i, state, T, pcm_format=fmt, hold=None)
        zero = dev.lc_decode_streams(channels, d_c, d_i, state, T, pcm_format=fmt,
                                     hold=torch.zeros(S * T, dtype=torch.uint8, device="cuda"))
        for other, name in ((none, "hold=None"), (zero, "all-zero mask")):
            _same(other[0], plain[0], name + " PCM")
            _same(other[1], plain[1], name + " state")


# ---------------------------------------------------------------------------------------------------------------
# HE-AAC
# ---------------------------------------------------------------------------------------------------------------
def _he_inputs(pkg, dev, cfg, S, T, seed, hdr, downsampled):
    import torch
    rng = np.random.default_rng(seed)
    frs = list(_synth().he_stream(rng, cfg, S, T + 1, hdr, ps_mode="mix", hdr_choice=np.arange(S) % len(hdr)))
    fr = {k: np.stack([f[k] for f in frs], axis=1) for k in ("coeffs", "ics", "sbr")}
    fr["ps"] = np.stack([f["ps"] for f in frs], axis=1) if cfg == pkg.CFG_HEV2 else None
    d_hdr = pkg.to_device(hdr)
    _, state = _he_step(pkg, dev, cfg, fr, 0, d_hdr, torch.zeros((S, pkg.STATE_WORDS[cfg]), device="cuda"), pkg.PCM_F32,
                        downsampled)
    return {k: (v[:, 1:] if v is not None else None) for k, v in fr.items()}, d_hdr, state


def _he_step(pkg, dev, cfg, fr, t, d_hdr, state, fmt, downsampled):
    ps = pkg.to_device(np.ascontiguousarray(fr["ps"][:, t])) if fr["ps"] is not None else None
    return dev.he_decode(cfg, _t(fr["coeffs"][:, t]), pkg.to_device(np.ascontiguousarray(fr["ics"][:, t])),
                         pkg.to_device(np.ascontiguousarray(fr["sbr"][:, t])), d_hdr, ps, state, pcm_format=fmt,
                         downsampled=downsampled)


def _he_reference(pkg, dev, cfg, fr, d_hdr, state, mask, fmt, downsampled):
    import torch
    S, T = mask.shape
    held = torch.from_numpy(mask != 0).cuda()
    state = state.clone()
    pcms = []
    for t in range(T):
        before = state.clone()
        pcm, state = _he_step(pkg, dev, cfg, fr, t, d_hdr, before, fmt, downsampled)
        state[held[:, t]] = before[held[:, t]]
        pcm[held[:, t]] = 0
        pcms.append(pcm)
    return torch.stack(pcms, dim=1), state


def _he_streams(pkg, dev, cfg, fr, d_hdr, state, state_out, mask, fmt, downsampled, T, hold=True):
    ps = _poisoned(fr["ps"], mask)
    return dev.he_decode_streams(cfg, _t(_poisoned(fr["coeffs"], mask)), pkg.to_device(_poisoned(fr["ics"], mask)),
                                 pkg.to_device(_poisoned(fr["sbr"], mask)), d_hdr,
                                 pkg.to_device(ps) if ps is not None else None, state, T, state_out=state_out,
                                 pcm_format=fmt, downsampled=downsampled, hold=_t(_flat(mask)) if hold else None)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("fmtname", ["PCM_F32", "PCM_S16", "PCM_S16_SSE2"])
@pytest.mark.parametrize("downsampled", [False, True])
@pytest.mark.parametrize("cfgname", ["CFG_HEV2", "CFG_HEV1", "CFG_HEV1_MONO"])
def test_he_streams_hold(pkg, dev, cfgname, downsampled, fmtname, T):
    import torch
    cfg, fmt = getattr(pkg, cfgname), getattr(pkg, fmtname)
    hdr = _synth().default_headers(pkg, extra=True)
    # S odd: mono cores pair two streams per wave.  On the default device (a workspace chunk of 64 frames) T = 8 gives 8
    # streams per chunk, so the call walks two chunks and the mask is taken at each chunk's offset
    S = 11
    fr, d_hdr, state = _he_inputs(pkg, dev, cfg, S, T, 500 + T, hdr, downsampled)
    for kind in MASKS:
        mask = _mask(kind, S, T, 23 * T + cfg)
        ref_pcm, ref_state = _he_reference(pkg, dev, cfg, fr, d_hdr, state, mask, fmt, downsampled)
        st_out = torch.full_like(state, 7.0)
        pcm, st = _he_streams(pkg, dev, cfg, fr, d_hdr, state, st_out, mask, fmt, downsampled, T)
        torch.cuda.synchronize()
        _same(pcm.reshape(ref_pcm.shape), ref_pcm, "%s PCM" % kind)
        _same(st, ref_state, "%s state" % kind)
        if kind == "all":
            _same(st, state, "all held: state_out is state_in")
            assert not bool(pcm.view(torch.uint8).any()), "all held: PCM is zero bytes"
        st_io = state.clone()
        pcm, _ = _he_streams(pkg, dev, cfg, fr, d_hdr, st_io, st_io, mask, fmt, downsampled, T)
        _same(pcm.reshape(ref_pcm.shape), ref_pcm, "%s PCM, in place" % kind)
        _same(st_io, ref_state, "%s state, in place" % kind)


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("cfgname", ["CFG_HEV2", "CFG_HEV1", "CFG_HEV1_MONO"])
def test_he_streams_no_mask_and_zero_mask_are_the_plain_call(pkg, dev, cfgname, T):
    import torch
    cfg = getattr(pkg, cfgname)
    hdr = _synth().default_headers(pkg)
    S = 7
    fr, d_hdr, state = _he_inputs(pkg, dev, cfg, S, T, 550 + T, hdr, False)
    zero = np.zeros((S, T), np.uint8)
    for fmt, ds in ((pkg.PCM_F32, False), (pkg.PCM_S16, False), (pkg.PCM_S16, True)):
        ps = pkg.to_device(_flat(fr["ps"])) if fr["ps"] is not None else None
        plain = dev.he_decode_streams(cfg, _t(_flat(fr["coeffs"])), pkg.to_device(_flat(fr["ics"])),
                                      pkg.to_device(_flat(fr["sbr"])), d_hdr, ps, state, T, pcm_format=fmt, downsampled=ds)
        none = _he_streams(pkg, dev, cfg, fr, d_hdr, state, None, zero, fmt, ds, T, hold=False)
        zeroed = _he_streams(pkg, dev, cfg, fr, d_hdr, state, None, zero, fmt, ds, T)
        for other, name in ((none, "hold=None"), (zeroed, "all-zero mask")):
            _same(other[0], plain[0], name + " PCM")
            _same(other[1], plain[1], name + " state")


# ---------------------------------------------------------------------------------------------------------------
# spectral tools
# ---------------------------------------------------------------------------------------------------------------
STATES = ("none", "pns", "main", "pns_main")


def _tools_inputs(pkg, S, T, channels, state, seed):
    rng = np.random.default_rng(seed)
    tools = np.stack([_synth().tools_frames(rng, pkg, S, channels) for _ in range(T)], axis=1)
    coeffs = np.stack([(rng.standard_normal((S, channels, 1024)) * 1e-4).astype(np.float32) for _ in range(T)], axis=1)
    rs = rng.integers(-2**31, 2**31, S).astype(np.int32) if "pns" in state else None
    pred = None
    if "main" in state:
        p = np.zeros((S, channels, pkg.MAX_PREDICTORS), pkg.PRED_STATE_DT)      # reset_all_predictors: cor = r = 0, var = 1
        p["var0"] = 1.0
        p["var1"] = 1.0
        pred = np.ascontiguousarray(p.view(np.float32).reshape(S, channels, pkg.MAX_PREDICTORS, 6))
    return coeffs, tools, rs, pred


def _tools_reference(pkg, dev, channels, coeffs, tools, rs, pred, mask):
    import torch
    S, T = mask.shape
    held = torch.from_numpy(mask != 0).cuda()
    d_rs = _t(rs) if rs is not None else None
    d_pred = _t(pred) if pred is not None else None
    out = []
    for t in range(T):
        rs0 = d_rs.clone() if d_rs is not None else None
        pred0 = d_pred.clone() if d_pred is not None else None
        d = _t(coeffs[:, t])
        dev.spectral_tools(channels, d, pkg.to_device(np.ascontiguousarray(tools[:, t])), rng=d_rs, pred=d_pred)
        if d_rs is not None:
            d_rs[held[:, t]] = rs0[held[:, t]]
        if d_pred is not None:
            d_pred[held[:, t]] = pred0[held[:, t]]
        out.append(d)
    return torch.stack(out, dim=1), d_rs, d_pred


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_hold(pkg, dev, channels, state, T):
    import torch
    S = 11
    coeffs, tools, rs, pred = _tools_inputs(pkg, S, T, channels, state, 700 + T + 10 * channels)
    for kind in MASKS:
        mask = _mask(kind, S, T, 29 * T + channels)
        run = torch.from_numpy(mask == 0).cuda()
        ref_c, ref_rs, ref_pred = _tools_reference(pkg, dev, channels, coeffs, tools, rs, pred, mask)
        for separate in (False, True):
            d_c = _t(_poisoned(coeffs, mask))
            d_rs = _t(rs) if rs is not None else None
            d_pred = _t(pred) if pred is not None else None
            kw = {}
            if separate:
                kw = dict(rng_out=torch.full_like(d_rs, 7) if rs is not None else None,
                          pred_out=torch.full_like(d_pred, 7.0) if pred is not None else None)
            dev.spectral_tools_streams(channels, d_c, pkg.to_device(_poisoned(tools, mask)), T, rng=d_rs, pred=d_pred,
                                       hold=_t(_flat(mask)), **kw)
            torch.cuda.synchronize()
            what = "%s%s" % (kind, ", separate state" if separate else "")
            # the frames that are not held (a held frame's coefficient row is unspecified)
            _same(d_c.reshape(ref_c.shape)[run], ref_c[run], what + " coefficients")
            if rs is not None:
                _same(kw["rng_out"] if separate else d_rs, ref_rs, what + " generator")
                if separate:
                    _same(d_rs, _t(rs), what + " generator input")
            if pred is not None:
                _same(kw["pred_out"] if separate else d_pred, ref_pred, what + " predictors")
            if kind == "all":
                if rs is not None:
                    _same(ref_rs, _t(rs), "all held: generator")
                if pred is not None:
                    _same(ref_pred, _t(pred), "all held: predictors")


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("state", STATES)
def test_tools_streams_no_mask_and_zero_mask_are_the_plain_call(pkg, dev, state, T):
    import torch
    S, channels = 9, 2
    coeffs, tools, rs, pred = _tools_inputs(pkg, S, T, channels, state, 750 + T)

    def call(**kw):
        d_c = _t(_flat(coeffs))
        d_rs = _t(rs) if rs is not None else None
        d_pred = _t(pred) if pred is not None else None
        dev.spectral_tools_streams(channels, d_c, pkg.to_device(_flat(tools)), T, rng=d_rs, pred=d_pred, **kw)
        return [x for x in (d_c, d_rs, d_pred) if x is not None]

    plain = call()
    for other, name in ((call(hold=None), "hold=None"),
                        (call(hold=torch.zeros(S * T, dtype=torch.uint8, device="cuda")), "all-zero mask")):
        for a, b in zip(other, plain):
            _same(a, b, name)
