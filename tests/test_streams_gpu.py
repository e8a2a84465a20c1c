"""heaac_he_decode_streams (S streams x T consecutive frames in one call) on the GPU: every PCM word and the final state
bit-exact against the oracle chained frame by frame, and word for word against T chained he_decode calls."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _synth():
    return importlib.import_module("ffmpeg_heaac_amd.synth")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _mismatch(a, b):
    d = _bits(a) != _bits(b)
    return int(d.sum()), (np.argwhere(d)[:5].tolist() if d.any() else [])


def _frames(pkg, cfg, S, steps, seed, hdr, ps_mode="20", hdr_choice=None, events=None):
    """he_stream steps stacked per stream: dict of arrays shaped [S][steps][...]."""
    rng = np.random.default_rng(seed)
    frs = list(_synth().he_stream(rng, cfg, S, steps, hdr, ps_mode=ps_mode, hdr_choice=hdr_choice, events=events))
    out = {k: np.stack([f[k] for f in frs], axis=1) for k in ("coeffs", "ics", "sbr")}
    out["ps"] = np.stack([f["ps"] for f in frs], axis=1) if cfg == pkg.CFG_HEV2 else None
    return out


def _flat(a, t0, t1):
    """frames t0..t1-1 of every stream, flattened to the streams layout (frame t of stream s at s * T + t)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a[:, t0:t1])
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


def _oracle_chain(pkg, oracle, cfg, fr, hdr, state, t0, t1, fmt, downsampled):
    """oracle.he_decode_batch frame position by frame position: PCM [S][T][...] and the state after t1 - 1"""
    pcms = []
    for t in range(t0, t1):
        ps = fr["ps"][:, t] if fr["ps"] is not None else None
        p, state = oracle.he_decode_batch(cfg, np.ascontiguousarray(fr["coeffs"][:, t]), np.ascontiguousarray(fr["ics"][:, t]),
                                          np.ascontiguousarray(fr["sbr"][:, t]), hdr,
                                          np.ascontiguousarray(ps) if ps is not None else None, state, fmt,
                                          downsampled=downsampled)
        pcms.append(p)
    return np.stack(pcms, axis=1), state


def _streams_call(pkg, dev, cfg, fr, hdr, state_in, t0, t1, fmt, downsampled=False, in_place=False):
    import torch
    T = t1 - t0
    d_state = torch.from_numpy(np.ascontiguousarray(state_in)).cuda()
    ps = _flat(fr["ps"], t0, t1)
    pcm, st = dev.he_decode_streams(cfg, torch.from_numpy(_flat(fr["coeffs"], t0, t1)).cuda(),
                                    pkg.to_device(_flat(fr["ics"], t0, t1)), pkg.to_device(_flat(fr["sbr"], t0, t1)),
                                    pkg.to_device(hdr), pkg.to_device(ps) if ps is not None else None, d_state, T,
                                    state_out=d_state if in_place else None, pcm_format=fmt, downsampled=downsampled)
    torch.cuda.synchronize()
    S = state_in.shape[0]
    return pcm.cpu().numpy().reshape((S, T) + tuple(pcm.shape[1:])), st.cpu().numpy()


def _check_vs_oracle(pkg, oracle, dev, cfg, S, T, seed, hdr, ps_mode="20", fmt=None, downsampled=False, in_place=False,
                     warm=1, hdr_choice=None, events=None):
    """`warm` frames through the oracle first (a state_in that is not all zeros), then T frames in one streams call"""
    fmt = pkg.PCM_F32 if fmt is None else fmt
    fr = _frames(pkg, cfg, S, warm + T, seed, hdr, ps_mode=ps_mode, hdr_choice=hdr_choice, events=events)
    state = np.zeros((S, pkg.STATE_WORDS[cfg]), np.float32)
    if warm:
        _, state = _oracle_chain(pkg, oracle, cfg, fr, hdr, state, 0, warm, fmt, downsampled)
    ref_pcm, ref_state = _oracle_chain(pkg, oracle, cfg, fr, hdr, state, warm, warm + T, fmt, downsampled)
    pcm, st = _streams_call(pkg, dev, cfg, fr, hdr, state, warm, warm + T, fmt, downsampled, in_place)
    nbad, where = _mismatch(pcm, ref_pcm) if fmt == pkg.PCM_F32 else (int((pcm != ref_pcm).sum()), None)
    assert nbad == 0, "%d PCM words differ, first at %s" % (nbad, where)
    nbad, where = _mismatch(st, ref_state)
    assert nbad == 0, "%d state words differ, first at %s" % (nbad, where)


CFGS = [("CFG_HEV1", "20"), ("CFG_HEV1_MONO", "20"), ("CFG_HEV2", "20"), ("CFG_HEV2", "34"), ("CFG_HEV2", "mix")]


@pytest.mark.parametrize("T", [1, 2, 3, 8])
@pytest.mark.parametrize("cfgname,ps_mode", CFGS)
def test_streams_match_oracle(pkg, oracle, dev, cfgname, ps_mode, T):
    hdr = _synth().default_headers(pkg, extra=True)
    S = 7                                            # odd: an odd count of core channel chains for the mono configs
    _check_vs_oracle(pkg, oracle, dev, getattr(pkg, cfgname), S, T, 100 + T, hdr, ps_mode=ps_mode,
                     hdr_choice=np.arange(S) % len(hdr))


@pytest.mark.parametrize("fmtname", ["PCM_S16", "PCM_S16_SSE2"])
@pytest.mark.parametrize("cfgname,ps_mode", [("CFG_HEV1", "20"), ("CFG_HEV1_MONO", "20"), ("CFG_HEV2", "mix")])
def test_streams_s16_formats(pkg, oracle, dev, cfgname, ps_mode, fmtname):
    hdr = _synth().default_headers(pkg)
    _check_vs_oracle(pkg, oracle, dev, getattr(pkg, cfgname), 5, 3, 7, hdr, ps_mode=ps_mode, fmt=getattr(pkg, fmtname))


@pytest.mark.parametrize("fmtname", ["PCM_F32", "PCM_S16", "PCM_S16_SSE2"])
@pytest.mark.parametrize("cfgname,ps_mode", [("CFG_HEV1", "20"), ("CFG_HEV1_MONO", "20"), ("CFG_HEV2", "mix")])
def test_streams_downsampled(pkg, oracle, dev, cfgname, ps_mode, fmtname):
    hdr = _synth().default_headers(pkg)
    _check_vs_oracle(pkg, oracle, dev, getattr(pkg, cfgname), 5, 4, 11, hdr, ps_mode=ps_mode, fmt=getattr(pkg, fmtname),
                     downsampled=True)


def test_streams_ps_layout_switches_inside_a_call(pkg, oracle, dev, monkeypatch):
    """Each stream's PS layout changes from frame to frame between baseline (20 bands, no IPD/OPD) and 34 bands with
    IPD/OPD, and PS drops out (start = 0) on some frames: the baseline frames go through the fused HF + PS kernel, the
    others through the general PS kernel, and the PS state chain crosses between them inside one call."""
    synth = _synth()
    base = synth._PsChain
    rng = np.random.default_rng(3)

    class Switching(base):
        def step(self, out):
            self.mode = "20" if rng.random() < 0.5 else "34"
            super().step(out)

    monkeypatch.setattr(synth, "_PsChain", Switching)
    hdr = synth.default_headers(pkg)
    _check_vs_oracle(pkg, oracle, dev, pkg.CFG_HEV2, 9, 8, 41, hdr, events=dict(p_ps_off=0.2))
    _check_vs_oracle(pkg, oracle, dev, pkg.CFG_HEV2, 9, 8, 42, hdr, fmt=pkg.PCM_S16, events=dict(p_ps_off=0.2))


@pytest.mark.parametrize("cfgname,ps_mode", [("CFG_HEV1", "20"), ("CFG_HEV2", "mix")])
def test_streams_in_place(pkg, oracle, dev, cfgname, ps_mode):
    hdr = _synth().default_headers(pkg)
    _check_vs_oracle(pkg, oracle, dev, getattr(pkg, cfgname), 6, 5, 13, hdr, ps_mode=ps_mode, in_place=True)
    _check_vs_oracle(pkg, oracle, dev, getattr(pkg, cfgname), 6, 5, 14, hdr, ps_mode=ps_mode, in_place=True,
                     downsampled=True)


def test_streams_degraded_paths(pkg, oracle, dev):
    """SBR header switches, dropped SBR payloads and lead-in frames before the first header, inside the chains."""
    synth = _synth()
    hdr = synth.default_headers(pkg, extra=True, null=True)
    ev = dict(lead_in=3, p_switch=0.2, p_drop=0.1, p_ps_off=0.1)
    for cfg, ps_mode in ((pkg.CFG_HEV1, "20"), (pkg.CFG_HEV2, "mix")):
        _check_vs_oracle(pkg, oracle, dev, cfg, 11, 6, 17, hdr, ps_mode=ps_mode, warm=0, events=ev)


def test_streams_several_chunks(pkg, oracle):
    """chunk = 256 frames: 32 streams of T = 8 per workspace set, 250 streams = 8 chunks on one lane"""
    d = pkg.Device(max_frames=256)
    try:
        hdr = _synth().default_headers(pkg)
        _check_vs_oracle(pkg, oracle, d, pkg.CFG_HEV2, 250, 8, 19, hdr, ps_mode="mix", warm=0)
    finally:
        d.close()


def test_streams_long_chain(pkg, oracle):
    """150 consecutive frames per stream in one call"""
    d = pkg.Device(max_frames=1024)
    try:
        hdr = _synth().default_headers(pkg)
        _check_vs_oracle(pkg, oracle, d, pkg.CFG_HEV2, 5, 150, 23, hdr, ps_mode="mix", warm=0, fmt=pkg.PCM_S16)
        _check_vs_oracle(pkg, oracle, d, pkg.CFG_HEV1, 3, 150, 24, hdr, warm=0)
    finally:
        d.close()


def test_streams_two_lanes_match_chained_batch_calls(pkg, oracle):
    """Device(max_frames=320 000): chunk 262 144, two workspace sets on two lanes.  S = 40 000 streams of T = 8 in one
    call against eight chained he_decode calls (product against product), and the oracle on a seeded sample."""
    import torch
    cfg, T, S, base_streams = pkg.CFG_HEV2, 8, 40000, 400
    hdr = _synth().default_headers(pkg)
    fr = _frames(pkg, cfg, base_streams, T, 29, hdr, ps_mode="mix")
    rep = S // base_streams
    d_hdr = pkg.to_device(hdr)
    d = pkg.Device(max_frames=320000)
    try:
        # streams form: stream s is base stream s % base_streams
        flat = {k: np.tile(_flat(fr[k], 0, T).reshape((base_streams, T) + fr[k].shape[2:]), (rep,) + (1,) * (fr[k].ndim - 1))
                for k in ("coeffs", "ics", "sbr", "ps")}
        st0 = torch.zeros((S, pkg.STATE_WORDS[cfg]), device="cuda")
        pcm_s, st_s = d.he_decode_streams(
            cfg, torch.from_numpy(flat["coeffs"].reshape((S * T,) + fr["coeffs"].shape[2:])).cuda(),
            pkg.to_device(flat["ics"].reshape((S * T,) + fr["ics"].shape[2:])),
            pkg.to_device(flat["sbr"].reshape(S * T)), d_hdr, pkg.to_device(flat["ps"].reshape(S * T)), st0, T,
            pcm_format=pkg.PCM_S16)
        # eight chained batch calls over the same frames
        st = torch.zeros_like(st0)
        pcm_b = torch.empty((S, T, 2048, 2), dtype=torch.int16, device="cuda")
        for t in range(T):
            col = {k: np.ascontiguousarray(flat[k][:, t]) for k in flat}
            p, st = d.he_decode(cfg, torch.from_numpy(col["coeffs"]).cuda(), pkg.to_device(col["ics"]),
                                pkg.to_device(col["sbr"]), d_hdr, pkg.to_device(col["ps"]), st, pcm_format=pkg.PCM_S16)
            pcm_b[:, t] = p
        torch.cuda.synchronize()
        assert torch.equal(pcm_s.view(S, T, 2048, 2), pcm_b)
        assert torch.equal(st_s.view(torch.int32), st.view(torch.int32))
        # the oracle on a sample of the base streams (each appears rep times; check the copies from the last chunk)
        pick = np.random.default_rng(31).choice(base_streams, 6, replace=False)
        sub = {k: fr[k][pick] for k in ("coeffs", "ics", "sbr", "ps")}
        ref_pcm, ref_state = _oracle_chain(pkg, oracle, cfg, sub, hdr, np.zeros((6, pkg.STATE_WORDS[cfg]), np.float32),
                                           0, T, pkg.PCM_S16, False)
        rows = (rep - 1) * base_streams + pick
        got = pcm_s.view(S, T, 2048, 2)[torch.from_numpy(rows).cuda()].cpu().numpy()
        assert np.array_equal(got, ref_pcm)
        nbad, where = _mismatch(st_s[torch.from_numpy(rows).cuda()].cpu().numpy(), ref_state)
        assert nbad == 0, where
    finally:
        d.close()


@pytest.mark.parametrize("cfgname,ps_mode", [("CFG_HEV1", "20"), ("CFG_HEV1_MONO", "20"), ("CFG_HEV2", "mix")])
def test_streams_t1_equals_batch_call(pkg, dev, cfgname, ps_mode):
    import torch
    cfg = getattr(pkg, cfgname)
    hdr = _synth().default_headers(pkg)
    S = 33
    fr = _frames(pkg, cfg, S, 2, 37, hdr, ps_mode=ps_mode)
    d_hdr = pkg.to_device(hdr)
    st = torch.zeros((S, pkg.STATE_WORDS[cfg]), device="cuda")
    ps = lambda t: pkg.to_device(np.ascontiguousarray(fr["ps"][:, t])) if fr["ps"] is not None else None
    args = lambda t: (torch.from_numpy(np.ascontiguousarray(fr["coeffs"][:, t])).cuda(),
                      pkg.to_device(np.ascontiguousarray(fr["ics"][:, t])),
                      pkg.to_device(np.ascontiguousarray(fr["sbr"][:, t])), d_hdr, ps(t))
    _, st = dev.he_decode(cfg, *args(0), st)                  # a state that is not all zeros
    for fmt in (pkg.PCM_F32, pkg.PCM_S16):
        for ds in (False, True):
            pb, sb = dev.he_decode(cfg, *args(1), st, pcm_format=fmt, downsampled=ds)
            ps_, ss = dev.he_decode_streams(cfg, *args(1), st, 1, pcm_format=fmt, downsampled=ds)
            torch.cuda.synchronize()
            assert torch.equal(pb.view(-1).view(torch.int16), ps_.view(-1).view(torch.int16)), (fmt, ds)
            assert torch.equal(sb.view(torch.int32), ss.view(torch.int32)), (fmt, ds)


def test_streams_argument_errors(pkg, dev):
    import torch
    cfg = pkg.CFG_HEV1_MONO
    hdr = pkg.to_device(_synth().default_headers(pkg))
    st = torch.zeros((2, pkg.STATE_WORDS[cfg]), device="cuda")

    def call(T):
        n = 2 * T
        return dev.he_decode_streams(cfg, torch.zeros((n, 1, 1024), device="cuda"),
                                     torch.zeros(n * pkg.ICS_DT.itemsize, dtype=torch.uint8, device="cuda"),
                                     torch.zeros(n * pkg.SBR_FRAME_DT.itemsize, dtype=torch.uint8, device="cuda"),
                                     hdr, None, st, T)
    for T in (0, 65):                                 # the default device's chunk is 64 frames
        with pytest.raises(pkg.HeaacError, match=r"\(-1\)"):
            call(T)
    # no streams: nothing to do
    pcm, st_out = dev.he_decode_streams(cfg, torch.zeros((0, 1, 1024), device="cuda"),
                                        torch.zeros(0, dtype=torch.uint8, device="cuda"),
                                        torch.zeros(0, dtype=torch.uint8, device="cuda"), hdr, None,
                                        torch.zeros((0, pkg.STATE_WORDS[cfg]), device="cuda"), 4)
    assert pcm.numel() == 0


def test_streams_graph_capture(pkg, oracle, dev):
    import torch
    synth = _synth()
    hdr = synth.default_headers(pkg)
    cfg, S, T = pkg.CFG_HEV2, 6, 4
    fr = _frames(pkg, cfg, S, T, 43, hdr, ps_mode="mix")
    ref_pcm, ref_state = _oracle_chain(pkg, oracle, cfg, fr, hdr, np.zeros((S, pkg.STATE_WORDS[cfg]), np.float32),
                                       0, T, pkg.PCM_S16, False)
    args = (torch.from_numpy(_flat(fr["coeffs"], 0, T)).cuda(), pkg.to_device(_flat(fr["ics"], 0, T)),
            pkg.to_device(_flat(fr["sbr"], 0, T)), pkg.to_device(hdr), pkg.to_device(_flat(fr["ps"], 0, T)))
    st_in = torch.zeros((S, pkg.STATE_WORDS[cfg]), device="cuda")
    st_out = torch.empty_like(st_in)
    pcm = torch.empty((S * T, 2048, 2), dtype=torch.int16, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev.he_decode_streams(cfg, *args, st_in, T, state_out=st_out, pcm=pcm, pcm_format=pkg.PCM_S16)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dev.he_decode_streams(cfg, *args, st_in, T, state_out=st_out, pcm=pcm, pcm_format=pkg.PCM_S16)
    pcm.zero_(); st_out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(pcm.cpu().numpy().reshape(ref_pcm.shape), ref_pcm)
    nbad, where = _mismatch(st_out.cpu().numpy(), ref_state)
    assert nbad == 0, where


def test_x_band_records_past_one_chunk_are_the_frames_in_order(pkg):
    """heaac_debug_xbands for a call of two chunks on two lanes (bench.py asks for it after the timed work of any
    --frames above 262 144): Device(max_frames=300 000) decodes 300 000 HE-AACv2 frames with mixed headers in one call,
    and the hook's 600 000 bytes equal the records of the same frames decoded in two calls of at most one chunk.
    More frames than the device holds records for (two sets of one chunk) are an argument error."""
    import torch
    cfg, n, base, chunk = pkg.CFG_HEV2, 300000, 1000, 262144
    hdr = _synth().default_headers(pkg)
    fr = _frames(pkg, cfg, base, 2, 43, hdr, ps_mode="mix")
    flat = {k: np.tile(fr[k][:, 1], (n // base,) + (1,) * (fr[k].ndim - 2)) for k in ("coeffs", "ics", "sbr", "ps")}
    d_hdr = pkg.to_device(hdr)
    d = pkg.Device(max_frames=n)
    try:
        def run(lo, hi):
            col = {k: np.ascontiguousarray(flat[k][lo:hi]) for k in flat}
            st = torch.zeros((hi - lo, pkg.STATE_WORDS[cfg]), device="cuda")
            d.he_decode(cfg, torch.from_numpy(col["coeffs"]).cuda(), pkg.to_device(col["ics"]), pkg.to_device(col["sbr"]),
                        d_hdr, pkg.to_device(col["ps"]), st, state_out=st, pcm_format=pkg.PCM_S16)
            torch.cuda.synchronize()
            return d.x_bands(hi - lo)
        whole = run(0, n)
        parts = np.concatenate([run(0, chunk), run(chunk, n)])
        assert whole.shape == (n, 2) and whole.tobytes() == parts.tobytes()
        assert set(np.unique(whole).tolist()) <= {32, 48, 64}
        # the frames of the first chunk are the first frames of the call, those of the second follow
        assert np.array_equal(whole[chunk:], run(chunk, n))
        assert d.x_bands(2 * chunk).shape == (2 * chunk, 2)
        with pytest.raises(pkg.HeaacError):
            d.x_bands(2 * chunk + 1)
    finally:
        d.close()
