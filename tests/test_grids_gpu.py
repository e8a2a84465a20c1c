"""GPU parity over the structure the C ABI accepts: the profiles of tests/edge_grids.py (five envelopes on every
pointer and the widest limiter table; one-slot envelopes, the longest and the shortest frame; frames that start after
or before the end of the last one, with and without a reset, with and without smoothing; records drawn uniformly over
what csrc/validate.h accepts; PS grids with every border at 8k - 1 but uneven, one-slot and five-envelope PS grids,
free PS carries; every window-sequence and window-shape transition) against the oracle chained frame by frame.
tests/test_grid_reach.py shows, on the CPU, that these inputs hold the classes they are for, and that the oracle is
defined on them.

Bar: the project's own (tests/test_edges_gpu.py): f32 PCM words and every state word bit-identical to the oracle,
int16 identical; a NaN of the oracle would be matched by any NaN (these profiles stay finite).  No tolerance."""
import importlib

import numpy as np
import pytest

import edge_grids as G
from test_edges_gpu import _check_pcm, assert_words

pytestmark = pytest.mark.gpu

FMTS = ("PCM_F32", "PCM_S16")


def _synth():
    return importlib.import_module("ffmpeg_heaac_amd.synth")


def _he_both_forms(pkg, oracle, dev, cfg, fmt, ds, hdr, frames):
    """he_decode chained frame by frame with the state in place, and the same frames in one he_decode_streams call
    with T = all frames (the carry of the rings and of the grid's old border stays on chip), both against the oracle
    chained frame by frame"""
    import torch
    n, T = frames[0]["coeffs"].shape[0], len(frames)
    state = np.zeros((n, pkg.STATE_WORDS[cfg]), np.float32)
    d_state = torch.from_numpy(state).cuda()
    d_hdr = pkg.to_device(hdr)
    ref_pcm = []
    for t, fr in enumerate(frames):
        ref, state = oracle.he_decode_batch(cfg, fr["coeffs"], fr["ics"], fr["sbr"], hdr, fr["ps"], state, fmt,
                                            downsampled=ds)
        ref_pcm.append(ref)
        pcm, _ = dev.he_decode(cfg, torch.from_numpy(fr["coeffs"]).cuda(), pkg.to_device(fr["ics"]),
                               pkg.to_device(fr["sbr"]), d_hdr,
                               pkg.to_device(fr["ps"]) if fr["ps"] is not None else None, d_state, state_out=d_state,
                               pcm_format=fmt, downsampled=ds)
        _check_pcm(pkg, fmt, pcm.cpu().numpy(), ref, "he_decode frame %d PCM" % t)
        assert_words(d_state.cpu().numpy(), state, "he_decode frame %d state" % t)
    # frame t of stream s at s * T + t
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


@pytest.mark.parametrize("fmtname", FMTS)
@pytest.mark.parametrize("profile,cfgname,ps_mode,ds", G.cases())
def test_he_grids(pkg, oracle, dev, profile, cfgname, ps_mode, ds, fmtname):
    synth = _synth()
    cfg, fmt = getattr(pkg, cfgname), getattr(pkg, fmtname)
    hdr = G.headers(pkg, synth, profile)
    frames = G.he_frames(pkg, synth, cfg, profile, G.STREAMS, G.STEPS, G.SEED, hdr, ps_mode=ps_mode)
    _he_both_forms(pkg, oracle, dev, cfg, fmt, ds, hdr, frames)


@pytest.mark.parametrize("cfgname", ["CFG_HEV1", "CFG_HEV2"])
def test_he_core_windows(pkg, oracle, dev, cfgname):
    """every (window_sequence, previous) x (shape, previous shape) combination in the core of the HE kernels"""
    synth = _synth()
    cfg = getattr(pkg, cfgname)
    hdr = synth.default_headers(pkg, extra=True)
    _he_both_forms(pkg, oracle, dev, cfg, pkg.PCM_F32, False, hdr, G.he_window_frames(pkg, synth, cfg, G.SEED, hdr))


@pytest.mark.parametrize("fmtname", FMTS)
@pytest.mark.parametrize("channels", [1, 2])
def test_lc_windows(pkg, oracle, dev, channels, fmtname):
    """the same chains through lc_decode frame by frame and through one lc_decode_streams call"""
    import torch
    fmt = getattr(pkg, fmtname)
    frames = G.lc_window_frames(pkg, _synth(), channels, G.SEED)
    n, T = G.WIN_STREAMS, len(frames)
    state = np.zeros((n, channels * 512), np.float32)
    d_state = torch.from_numpy(state).cuda()
    ref_pcm = []
    for t, (coeffs, ics) in enumerate(frames):
        ref, state = oracle.lc_decode_batch(channels, coeffs, ics, state, fmt)
        ref_pcm.append(ref)
        pcm, d_state = dev.lc_decode(channels, torch.from_numpy(coeffs).cuda(), pkg.to_device(ics), d_state,
                                     pcm_format=fmt)
        _check_pcm(pkg, fmt, pcm.cpu().numpy(), ref, "lc frame %d PCM" % t)
        assert_words(d_state.cpu().numpy(), state, "lc frame %d state" % t)
    coeffs = np.ascontiguousarray(np.stack([c for c, _ in frames], axis=1).reshape(n * T, channels, 1024))
    ics = np.ascontiguousarray(np.stack([i for _, i in frames], axis=1).reshape(n * T, channels))
    pcm, st = dev.lc_decode_streams(channels, torch.from_numpy(coeffs).cuda(), pkg.to_device(ics),
                                    torch.zeros((n, channels * 512), dtype=torch.float32, device="cuda"), T,
                                    pcm_format=fmt)
    torch.cuda.synchronize()
    got = pcm.cpu().numpy().reshape((n, T) + tuple(pcm.shape[1:]))
    for t in range(T):
        _check_pcm(pkg, fmt, got[:, t], ref_pcm[t], "lc streams frame %d PCM" % t)
    assert_words(st.cpu().numpy(), state, "lc streams final state")
