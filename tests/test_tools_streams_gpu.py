"""heaac_spectral_tools_streams (S streams x T consecutive frames of the spectral tools in one call) on the GPU: every
coefficient, generator state and predictor word bit-exact against the oracle chained frame position by frame
position, and word for word against T chained spectral_tools calls."""
import ctypes as C
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

import edge_signals as E

pytestmark = pytest.mark.gpu

# the state a call carries: nothing, the noise generator, the AAC-Main predictors alone (d_rng_in NULL), both
STATES = ("none", "pns", "main", "pns_main")


def _synth():
    return importlib.import_module("ffmpeg_heaac_amd.synth")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_words(got, ref, what):
    """f32 words bit for bit; a NaN of the reference is matched by any NaN (DESIGN s2, tests/test_edges_gpu.py)"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    ok = (_bits(got) == _bits(ref)) | (np.isnan(got) & np.isnan(ref))
    assert ok.all(), "%s: %d words differ, first at %s" % (what, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


def _flat(a):
    return np.ascontiguousarray(a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:]))


def _reset_pred(pkg, S, channels):
    """reset_all_predictors (aacdec.c:507-522): cor = r = 0, var = 1"""
    p = np.zeros((S, channels, pkg.MAX_PREDICTORS), pkg.PRED_STATE_DT)
    p["var0"] = 1.0
    p["var1"] = 1.0
    return np.ascontiguousarray(p.view(np.float32).reshape(S, channels, pkg.MAX_PREDICTORS, 6))


def _frames(pkg, S, T, channels, seed, profile=None):
    """tools records [S][T] and spectra [S][T][channels][1024]"""
    rng = np.random.default_rng(seed)
    tools = np.stack([_synth().tools_frames(rng, pkg, S, channels) for _ in range(T)], axis=1)
    if profile is None:
        coeffs = np.stack([(rng.standard_normal((S, channels, 1024)) * 1e-4).astype(np.float32) for _ in range(T)],
                          axis=1)
    else:
        coeffs = np.stack([E.tools_coeffs(profile, rng, S, channels, t) for t in range(T)], axis=1)
    return np.ascontiguousarray(coeffs), np.ascontiguousarray(tools)


def _state(pkg, S, channels, state, seed):
    rng = np.random.default_rng(seed)
    rs = rng.integers(-2**31, 2**31, S).astype(np.int32) if "pns" in state else None
    if rs is not None:
        rs[0] = 0x1f2e3d4c                                    # ac->random_state at init
    pred = _reset_pred(pkg, S, channels) if "main" in state else None
    return rs, pred


def _oracle_chain(oracle, channels, coeffs, tools, rs, pred):
    """oracle.spectral_tools_batch frame position by frame position, the state chained"""
    out = np.empty_like(coeffs)
    for t in range(coeffs.shape[1]):
        r = oracle.spectral_tools_batch(channels, np.ascontiguousarray(coeffs[:, t]), np.ascontiguousarray(tools[:, t]),
                                        rs, pred)
        if rs is None and pred is None:
            out[:, t] = r
        elif pred is None:
            out[:, t], rs = r
        elif rs is None:
            out[:, t], pred = r
        else:
            out[:, t], rs, pred = r
    return out, rs, pred


def _dev_t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _streams(pkg, dev, channels, coeffs, tools, rs, pred, separate=False):
    """one streams call; returns (coeffs [S][T]..., rng_out, pred_out) on the host"""
    import torch
    S, T = coeffs.shape[:2]
    d = _dev_t(_flat(coeffs))
    d_rs, d_pred = _dev_t(rs), _dev_t(pred)
    kw = {}
    if separate:
        kw = dict(rng_out=None if rs is None else torch.full_like(d_rs, 7),
                  pred_out=None if pred is None else torch.full_like(d_pred, 7.0))
    dev.spectral_tools_streams(channels, d, pkg.to_device(_flat(tools)), T, rng=d_rs, pred=d_pred, **kw)
    torch.cuda.synchronize()
    if separate:
        if rs is not None:
            assert np.array_equal(d_rs.cpu().numpy(), rs), "rng input changed"
        if pred is not None:
            assert np.array_equal(_bits(d_pred.cpu().numpy()), _bits(pred)), "pred input changed"
        d_rs, d_pred = kw["rng_out"], kw["pred_out"]
    return (d.cpu().numpy().reshape(coeffs.shape), None if rs is None else d_rs.cpu().numpy(),
            None if pred is None else d_pred.cpu().numpy())


def _batch_chain(pkg, dev, channels, coeffs, tools, rs, pred):
    """T chained Device.spectral_tools calls on the GPU, each over the gathered frames of one position"""
    import torch
    out = np.empty_like(coeffs)
    d_rs, d_pred = _dev_t(rs), _dev_t(pred)
    for t in range(coeffs.shape[1]):
        d = _dev_t(coeffs[:, t])
        dev.spectral_tools(channels, d, pkg.to_device(np.ascontiguousarray(tools[:, t])), rng=d_rs, pred=d_pred)
        out[:, t] = d.cpu().numpy()
    torch.cuda.synchronize()
    return out, None if rs is None else d_rs.cpu().numpy(), None if pred is None else d_pred.cpu().numpy()


def _assert_same(got, ref, what=""):
    for k, name in enumerate(("coefficients", "rng_out", "pred_out")):
        if ref[k] is None:
            assert got[k] is None
        elif name == "rng_out":
            assert np.array_equal(got[k], ref[k]), what + name
        else:
            _assert_words(got[k], ref[k], what + name)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("T", [1, 2, 3, 8])
@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_match_oracle(pkg, oracle, dev, channels, T, state):
    S = 37
    coeffs, tools = _frames(pkg, S, T, channels, 100 * T + 10 * channels + STATES.index(state))
    rs, pred = _state(pkg, S, channels, state, T)
    ref = _oracle_chain(oracle, channels, coeffs, tools, rs, pred)
    got = _streams(pkg, dev, channels, coeffs, tools, rs, pred)
    _assert_same(got, ref)
    # coverage of the drawn batch
    ch = tools["ch"][:, :, :channels]
    assert (ch["band_type"] == 13).any()                                          # noise bands
    if T >= 3:                                                                    # a reset inside a chain ...
        eight = ch["ics"]["num_windows"][:, 1:T - 1] == 8
        assert eight.any()                                                        # ... with frames after it
    if T >= 2:
        assert (ch["pred"]["predictor_reset_group"][:, 1:] != 0).any()
    if pred is not None:
        assert (ref[2][..., 2] > 1).any()                                          # var0 > 1: predictors adapted
    if rs is not None:
        assert not np.array_equal(ref[1], rs)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("state", STATES[1:])
def test_tools_streams_equal_chained_batch_calls(pkg, dev, channels, state):
    S, T = 37, 5
    coeffs, tools = _frames(pkg, S, T, channels, 7 + channels)
    rs, pred = _state(pkg, S, channels, state, 3)
    _assert_same(_streams(pkg, dev, channels, coeffs, tools, rs, pred),
                 _batch_chain(pkg, dev, channels, coeffs, tools, rs, pred))


@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_stateless_equals_one_batch_call(pkg, dev, channels):
    S, T = 37, 4
    coeffs, tools = _frames(pkg, S, T, channels, 11 + channels)
    got = _streams(pkg, dev, channels, coeffs, tools, None, None)
    d = _dev_t(_flat(coeffs))
    dev.spectral_tools(channels, d, pkg.to_device(_flat(tools)))
    _assert_words(got[0].reshape(d.shape), d.cpu().numpy(), "coefficients")


@pytest.mark.parametrize("state", STATES[1:])
@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_in_place_and_separate_outputs(pkg, oracle, dev, channels, state):
    S, T = 9, 4
    coeffs, tools = _frames(pkg, S, T, channels, 21 + channels)
    rs, pred = _state(pkg, S, channels, state, 5)
    ref = _oracle_chain(oracle, channels, coeffs, tools, rs, pred)
    _assert_same(_streams(pkg, dev, channels, coeffs, tools, rs, pred), ref, "in place: ")
    _assert_same(_streams(pkg, dev, channels, coeffs, tools, rs, pred, separate=True), ref, "separate: ")


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_long_chain(pkg, oracle, dev, channels, S):
    T = 150
    coeffs, tools = _frames(pkg, S, T, channels, 31 + S + channels)
    rs, pred = _state(pkg, S, channels, "pns_main", 7)
    _assert_same(_streams(pkg, dev, channels, coeffs, tools, rs, pred),
                 _oracle_chain(oracle, channels, coeffs, tools, rs, pred))


def _tile_streams(coeffs, tools, S):
    """S streams from the drawn ones, repeated"""
    k = (S + coeffs.shape[0] - 1) // coeffs.shape[0]
    return (np.ascontiguousarray(np.tile(coeffs, (k, 1, 1, 1))[:S]),
            np.ascontiguousarray(np.tile(tools, (k, 1))[:S]))


@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_many_streams(pkg, dev, channels):
    """several thousand streams: the waves stride over them (grid capped at 256 workgroups)"""
    S, T = 5003, 4
    coeffs, tools = _tile_streams(*_frames(pkg, 97, T, channels, 41 + channels), S)
    rs, pred = _state(pkg, S, channels, "pns_main", 9)
    pred = pred + np.random.default_rng(2).standard_normal(pred.shape).astype(np.float32) * 0.01   # streams differ
    _assert_same(_streams(pkg, dev, channels, coeffs, tools, rs, pred),
                 _batch_chain(pkg, dev, channels, coeffs, tools, rs, pred))


@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_position_independent(pkg, dev, channels):
    S, T = 2600, 3
    coeffs, tools = _tile_streams(*_frames(pkg, 61, T, channels, 51 + channels), S)
    rs, pred = _state(pkg, S, channels, "pns_main", 11)
    pred[:, :, :, 2] += np.arange(S, dtype=np.float32)[:, None, None]            # var0: every stream its own
    allc, allr, allp = _streams(pkg, dev, channels, coeffs, tools, rs, pred)
    for s in (0, 1, 1279, 2560, S - 1):
        one = _streams(pkg, dev, channels, coeffs[s:s + 1], tools[s:s + 1], rs[s:s + 1], pred[s:s + 1])
        _assert_same(one, (allc[s:s + 1], allr[s:s + 1], allp[s:s + 1]), "stream %d " % s)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("profile", E.CORE_PROFILES)
def test_tools_streams_edges(pkg, oracle, dev, profile, channels):
    S, T = E.STREAMS + 1, E.min_steps(profile)
    coeffs, tools = _frames(pkg, S, T, channels, E.SEED + 3, profile=profile)
    rs = np.full(S, 0x1f2e3d4c, np.int32)
    pred = _reset_pred(pkg, S, channels)
    _assert_same(_streams(pkg, dev, channels, coeffs, tools, rs, pred),
                 _oracle_chain(oracle, channels, coeffs, tools, rs, pred))


@pytest.mark.parametrize("fmtname", ["PCM_F32", "PCM_S16"])
@pytest.mark.parametrize("channels", [1, 2])
def test_tools_streams_into_lc_decode_streams(pkg, oracle, dev, channels, fmtname):
    import torch
    fmt = getattr(pkg, fmtname)
    S, T = 13, 6
    rng = np.random.default_rng(60 + channels)
    steps = list(_synth().lc_stream(rng, S, T, channels))
    coeffs = np.ascontiguousarray(np.stack([c for c, _ in steps], axis=1))
    ics = np.ascontiguousarray(np.stack([i for _, i in steps], axis=1))
    _, tools = _frames(pkg, S, T, channels, 62 + channels)
    rs, pred = _state(pkg, S, channels, "pns_main", 13)
    state = (rng.standard_normal((S, channels * 512)) * 1e-3).astype(np.float32)
    # the oracle: tools then decode, frame position by frame position
    st, r, p, ref_pcm = state, rs, pred, []
    for t in range(T):
        c, r, p = oracle.spectral_tools_batch(channels, np.ascontiguousarray(coeffs[:, t]),
                                              np.ascontiguousarray(tools[:, t]), r, p)
        pcm, st = oracle.lc_decode_batch(channels, c, np.ascontiguousarray(ics[:, t]), st, fmt)
        ref_pcm.append(pcm)
    d = _dev_t(_flat(coeffs))
    d_rs, d_pred = _dev_t(rs), _dev_t(pred)
    dev.spectral_tools_streams(channels, d, pkg.to_device(_flat(tools)), T, rng=d_rs, pred=d_pred)
    pcm, d_st = dev.lc_decode_streams(channels, d, pkg.to_device(_flat(ics)), _dev_t(state), T, pcm_format=fmt)
    torch.cuda.synchronize()
    got = pcm.cpu().numpy().reshape((S, T) + tuple(pcm.shape[1:]))
    for t in range(T):
        if fmt == pkg.PCM_F32:
            _assert_words(got[:, t], ref_pcm[t], "frame %d PCM" % t)
        else:
            assert np.array_equal(got[:, t], ref_pcm[t]), "frame %d PCM" % t
    _assert_words(d_st.cpu().numpy(), st, "final state")
    assert np.array_equal(d_rs.cpu().numpy(), r)
    _assert_words(d_pred.cpu().numpy(), p, "pred_out")


@pytest.mark.parametrize("cfgname", ["CFG_HEV1", "CFG_HEV2"])
def test_tools_streams_into_he_decode_streams(pkg, oracle, dev, cfgname):
    import torch
    cfg = getattr(pkg, cfgname)
    synth = _synth()
    S, T = 6, 4
    hdr = synth.default_headers(pkg)
    frs = list(synth.he_stream(np.random.default_rng(70), cfg, S, T, hdr))
    channels = pkg.CORE_CH[cfg]

    def stack(k):
        return np.ascontiguousarray(np.stack([f[k] for f in frs], axis=1))
    coeffs, ics, sbr = stack("coeffs"), stack("ics"), stack("sbr")
    ps = stack("ps") if cfg == pkg.CFG_HEV2 else None
    _, tools = _frames(pkg, S, T, channels, 71)
    rs, pred = _state(pkg, S, channels, "pns", 15)
    state = np.zeros((S, pkg.STATE_WORDS[cfg]), np.float32)
    st, r, ref_pcm = state, rs, []
    for t in range(T):
        c, r = oracle.spectral_tools_batch(channels, np.ascontiguousarray(coeffs[:, t]),
                                           np.ascontiguousarray(tools[:, t]), r)
        pcm, st = oracle.he_decode_batch(cfg, c, np.ascontiguousarray(ics[:, t]), np.ascontiguousarray(sbr[:, t]), hdr,
                                         None if ps is None else np.ascontiguousarray(ps[:, t]), st, pkg.PCM_S16)
        ref_pcm.append(pcm)
    d = _dev_t(_flat(coeffs))
    d_rs = _dev_t(rs)
    dev.spectral_tools_streams(channels, d, pkg.to_device(_flat(tools)), T, rng=d_rs)
    pcm, d_st = dev.he_decode_streams(cfg, d, pkg.to_device(_flat(ics)), pkg.to_device(_flat(sbr)), pkg.to_device(hdr),
                                      None if ps is None else pkg.to_device(_flat(ps)), _dev_t(state), T,
                                      pcm_format=pkg.PCM_S16)
    torch.cuda.synchronize()
    got = pcm.cpu().numpy().reshape((S, T) + tuple(pcm.shape[1:]))
    for t in range(T):
        assert np.array_equal(got[:, t], ref_pcm[t]), "frame %d PCM" % t
    assert np.array_equal(d_rs.cpu().numpy(), r)


sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_bitstream_vectors as B  # noqa: E402


# noise bands in the units of each stored stream (the generator's work); none of them is an AAC-Main stream, so no
# unit has predictor_present and the predictors only run with output disabled
GOLDEN_NOISE_BANDS = {"lc_stereo_48k": 62, "hev1_stereo_24k": 12, "hev2_mono_24k": 0}


@pytest.mark.parametrize("name", sorted(GOLDEN_NOISE_BANDS))
def test_tools_streams_golden_bitstreams(pkg, dev, name):
    """the committed access units through the host parser one at a time, then S = 3 copies through the streams forms
    with T = all units, from the codec surface's start state: each stream's int16 PCM hashes to the stored value.
    lc_stereo_48k (62 noise bands in 8 units) and hev1_stereo_24k (12 in 8) run the generator; hev2_mono_24k has
    none.  No unit uses prediction."""
    import torch
    v = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bitstreams.json")))[name]
    asc, si, cpe, sbr, ps, frames, seed = B.STREAMS[name]
    ch = 2 if cpe else 1
    m4, _ = pkg.asc_parse(asc)
    if sbr:
        m4.sbr = 1
    if ps:
        m4.ps = 1
    hcfg = (pkg.CFG_HEV1 if cpe else pkg.CFG_HEV2) if sbr else (pkg.CFG_LC_STEREO if cpe else pkg.CFG_LC_MONO)
    tab = pkg.SbrHeaderTable(64)
    st, sst = np.zeros(1, pkg.AAC_STREAM_DT), pkg.sbr_streams(1)
    parsed = []
    for a in v["access_units"]:
        au = bytes.fromhex(a)
        p = (pkg.heaac_parse_batch(m4, st, sst, tab, [au], threads=1, with_ps=ps) if sbr
             else pkg.aac_parse_batch(m4, st, [au], threads=1))
        assert p["failed"] == 0
        parsed.append(p)
    T, S = len(parsed), 3

    def stack(get):
        x = np.concatenate([get(p) for p in parsed])                 # [T] ...
        return np.ascontiguousarray(np.broadcast_to(x, (S,) + x.shape).reshape((S * T,) + x.shape[1:]))
    coeffs = stack(lambda p: np.ascontiguousarray(p["coeffs"][:, :ch]))
    tools = stack(lambda p: p["tools"])
    ics = stack(lambda p: np.ascontiguousarray(p["ics"][:, :ch]))
    assert int((tools["ch"]["band_type"][:T, :ch] == 13).sum()) == GOLDEN_NOISE_BANDS[name]
    assert not tools["ch"]["pred"]["predictor_present"][:, :ch].any()
    d = _dev_t(coeffs)
    d_rs = torch.full((S,), 0x1f2e3d4c, dtype=torch.int32, device="cuda")
    d_pred = _dev_t(_reset_pred(pkg, S, ch))
    dev.spectral_tools_streams(ch, d, pkg.to_device(tools), T, rng=d_rs, pred=d_pred)
    state = torch.zeros((S, pkg.STATE_WORDS[hcfg] if sbr else ch * 512), device="cuda")
    if sbr:
        sbrr = stack(lambda p: p["sbr"])
        psr = pkg.to_device(stack(lambda p: p["ps"])) if ps else None
        pcm, _ = dev.he_decode_streams(hcfg, d, pkg.to_device(ics), pkg.to_device(sbrr), pkg.to_device(tab.headers()),
                                       psr, state, T, pcm_format=pkg.PCM_S16)
    else:
        pcm, _ = dev.lc_decode_streams(ch, d, pkg.to_device(ics), state, T, pcm_format=pkg.PCM_S16)
    torch.cuda.synchronize()
    out = pcm.cpu().numpy().reshape((S, T) + tuple(pcm.shape[1:]))
    assert list(out.shape[2:]) == v["frame_shape"]
    for s in range(S):
        assert hashlib.sha256(out[s].tobytes()).hexdigest() == v["pcm_s16_sha256"], "stream %d" % s


def test_tools_streams_argument_errors(pkg, dev):
    import torch
    f = pkg.lib().heaac_spectral_tools_streams
    buf = torch.zeros(4 * 2 * 1024, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    ERR = -1

    def call(channels=2, S=2, T=2, ptrs=None):
        ptrs = ptrs or [p] * 6
        return f(dev._h, channels, *ptrs, S, T, None)
    for ch in (0, 3, -1):
        assert call(channels=ch) == ERR
    assert call(T=0) == ERR
    assert call(S=0, T=0) == ERR
    for k in (0, 1):                                   # coefficients, records
        ptrs = [p] * 6
        ptrs[k] = None
        assert call(ptrs=ptrs) == ERR, k
    for k in (2, 4):                                   # an input state without its output
        ptrs = [p] * 6
        ptrs[k + 1] = None
        assert call(ptrs=ptrs) == ERR, k
        assert call(T=1, ptrs=ptrs) == ERR, k
    assert call(S=1 << 62, T=4) == ERR                 # S * T overflows
    assert call(S=1 << 45, T=1 << 10) == ERR           # S * T fits, S * T * channels * 1024 floats do not
    assert call(S=1 << 31, T=1 << 8, channels=1) == ERR   # records fit, k_tns's block count does not
    assert call(S=0, T=3) == 0                         # no streams: nothing to do
    assert call(S=0, T=3, ptrs=[None] * 6) == 0
    torch.cuda.synchronize()
    assert not buf.any()                               # nothing ran


def test_tools_streams_graph_capture(pkg, oracle, dev):
    import torch
    S, T, channels = 7, 4, 2
    rng = np.random.default_rng(80)
    steps = list(_synth().lc_stream(rng, S, T, channels))
    coeffs = np.ascontiguousarray(np.stack([c for c, _ in steps], axis=1))
    ics = np.ascontiguousarray(np.stack([i for _, i in steps], axis=1))
    _, tools = _frames(pkg, S, T, channels, 81)
    rs, pred = _state(pkg, S, channels, "pns_main", 17)
    state = np.zeros((S, channels * 512), np.float32)
    d_c0 = _dev_t(_flat(coeffs))
    d_c, d_tools, d_ics = d_c0.clone(), pkg.to_device(_flat(tools)), pkg.to_device(_flat(ics))
    rs_in, pred_in, st_in = _dev_t(rs), _dev_t(pred), _dev_t(state)
    rs_out, pred_out, st_out = torch.empty_like(rs_in), torch.empty_like(pred_in), torch.empty_like(st_in)
    pcm = torch.empty((S * T, 1024, channels), dtype=torch.int16, device="cuda")

    def run():
        dev.spectral_tools_streams(channels, d_c, d_tools, T, rng=rs_in, pred=pred_in, rng_out=rs_out,
                                   pred_out=pred_out)
        dev.lc_decode_streams(channels, d_c, d_ics, st_in, T, state_out=st_out, pcm=pcm, pcm_format=pkg.PCM_S16)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run()
        s.synchronize()
        eager = [x.cpu().numpy() for x in (pcm, st_out, rs_out, pred_out)]
        d_c.copy_(d_c0)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            run()
    d_c.copy_(d_c0)
    for x in (pcm, st_out, rs_out, pred_out):
        x.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    replay = [x.cpu().numpy() for x in (pcm, st_out, rs_out, pred_out)]
    assert np.array_equal(replay[0], eager[0])
    for a, b in zip(replay[1:], eager[1:]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                              b.view(np.uint32) if b.dtype == np.float32 else b)
    # and the eager run is the oracle's
    st, r, p, ref = state, rs, pred, []
    for t in range(T):
        c, r, p = oracle.spectral_tools_batch(channels, np.ascontiguousarray(coeffs[:, t]),
                                              np.ascontiguousarray(tools[:, t]), r, p)
        out, st = oracle.lc_decode_batch(channels, c, np.ascontiguousarray(ics[:, t]), st, pkg.PCM_S16)
        ref.append(out)
    assert np.array_equal(eager[0].reshape((S, T, 1024, channels)), np.stack(ref, axis=1))
    assert np.array_equal(eager[2], r)
