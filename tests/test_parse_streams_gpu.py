"""heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams on the GPU (k_parse_streams: one lane per stream, the
lane loops over its T units).  The model is the chained ONE-UNIT device calls, position by position, with the masking
and the put-back of parse_streams_common.model on the host; everything the contract specifies is byte-equal to it,
every output pre-filled with 0xA5.  Then the stop rule with neighbouring lanes stopping at different units, bytes to
PCM through the *_streams_ex calls with the parser's own hold mask, the call captured into a graph, and the argument
checks with a real device."""
import ctypes as C

import numpy as np
import pytest

import parse_device_common as PC
import parse_streams_common as PS
import sbr_device_common as SD
import test_parse as TP

pytestmark = pytest.mark.gpu
FILL = PC.FILL
SIZES = [1, 63, 64, 65, 130]     # one lane, a wave short by one, a full wave, a block plus one, a last block that is not full
TS = [1, 2, 3, 5]


def load(pkg, aus):
    import torch
    buf, off = pkg.pack_units(aus)
    return torch.from_numpy(np.concatenate([buf, np.zeros(4, np.uint8)])).cuda(), torch.from_numpy(off.astype(np.int32)).cuda()


class DevOne:
    """The one-unit forms on the device: heaac_aac_parse_device and heaac_sbr_parse_device."""

    def __init__(self, pkg, dev):
        self.pkg, self.dev = pkg, dev

    def aac(self, cfg, st, aus, cc):
        import torch
        pkg, n = self.pkg, len(aus)
        self.d_au, self.d_off = load(pkg, aus)
        d_st = pkg.to_device(st.copy())
        pre = {k: pkg.to_device(v) for k, v in PC.filled(pkg, n, cc).items()}
        out = self.dev.aac_parse(cfg, d_st, self.d_au, self.d_off, coeff_channels=cc, status=torch.full((n,), 7, dtype=torch.int32, device="cuda"), **pre)
        torch.cuda.synchronize()
        st[...] = d_st.cpu().numpy().view(pkg.AAC_STREAM_DT)
        self.d_info, self.d_status = out["info"], out["status"]
        return dict(coeffs=out["coeffs"].cpu().numpy(), ics=out["ics"].cpu().numpy().view(pkg.ICS_DT).reshape(n, cc),
                    tools=out["tools"].cpu().numpy().view(pkg.TOOLS_FRAME_DT), info=out["info"].cpu().numpy().view(pkg.AAC_INFO_DT),
                    status=out["status"].cpu().numpy())

    def sbr(self, cfg, sst, aus, info, hdr, status, with_ps):
        import torch
        pkg, n = self.pkg, len(aus)
        pre = {k: (pkg.to_device(v) if v is not None else None) for k, v in SD.filled(pkg, sst, n, with_ps).items()}
        out = self.dev.sbr_parse_device(cfg, pkg.to_device(sst), self.d_au, self.d_off, self.d_info, pkg.to_device(hdr),
                                        aac_status=self.d_status.clone(), sst_out=pre["sst"].view(-1), sbr=pre["sbr"], ps=pre["ps"],
                                        status=torch.full((n,), 7, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return dict(sst=out["sst"].cpu().numpy().reshape(n, -1), sbr=out["sbr"].cpu().numpy().view(pkg.SBR_FRAME_DT),
                    ps=out["ps"].cpu().numpy().view(pkg.PS_FRAME_DT) if with_ps else None, status=out["status"].cpu().numpy())


def streams_call(pkg, dev, cfg, st, rows, cc, sst=None, hdr=None, with_ps=False):
    """One streams call on the GPU from st / sst (numpy, left alone), every output 0xA5-filled.  Returns (records as
    numpy arrays incl. status, taken, hold and sst, the AAC states after the call, the device tensors)."""
    import torch
    T, S = len(rows), len(rows[0])
    n = S * T
    d_au, d_off = load(pkg, PS.flat(rows))
    d_st = pkg.to_device(st.copy())
    pre = PS.filled_streams(pkg, S, T, cc, sst, with_ps)
    pre.pop("why")
    pre["taken"] = pre["taken"].view(np.int32)
    d = {k: (pkg.to_device(v) if v is not None else None) for k, v in pre.items()}
    aac = dict(coeffs=d["coeffs"].view(-1), ics=d["ics"], tools=d["tools"], info=d["info"], status=d["status"], taken=d["taken"], hold=d["hold"])
    if sst is None:
        out = dev.aac_parse_streams(cfg, d_st, d_au, d_off, T, coeff_channels=cc, **aac)
    else:
        d_in = pkg.to_device(sst)
        out = dev.heaac_parse_device_streams(cfg, d_st, d_in, d_au, d_off, pkg.to_device(hdr), T, coeff_channels=cc,
                                             sst_out=d["sst"].view(-1), sbr=d["sbr"], ps=d["ps"], **aac)
    torch.cuda.synchronize()
    got = dict(coeffs=out["coeffs"].cpu().numpy(), ics=out["ics"].cpu().numpy().view(pkg.ICS_DT).reshape(n, cc),
               tools=out["tools"].cpu().numpy().view(pkg.TOOLS_FRAME_DT), info=out["info"].cpu().numpy().view(pkg.AAC_INFO_DT),
               status=out["status"].cpu().numpy(), taken=out["taken"].cpu().numpy().view(np.uint32), hold=out["hold"].cpu().numpy())
    if sst is not None:
        assert np.array_equal(d_in.cpu().numpy().reshape(S, -1), sst), "the in rows were written"
        got.update(sst=out["sst"].cpu().numpy().reshape(S, -1), sbr=out["sbr"].cpu().numpy().view(pkg.SBR_FRAME_DT),
                   ps=out["ps"].cpu().numpy().view(pkg.PS_FRAME_DT) if with_ps else None)
    return got, d_st.cpu().numpy().view(pkg.AAC_STREAM_DT), out


def run(pkg, dev, cfg, st, rows, cc, sst=None, hdr=None, with_ps=False):
    """The call against the device model and against the host form's verdicts.  Returns (got, states after, model)."""
    T, S = len(rows), len(rows[0])
    mdl = PS.model(pkg, DevOne(pkg, dev), cfg, st, rows, cc, sst, hdr, with_ps)
    got, after, _ = streams_call(pkg, dev, cfg, st, rows, cc, sst, hdr, with_ps)
    PS.compare_with_model(pkg, got, after, mdl, S, T)
    host_st = st.copy()
    host = pkg.parse_core_streams(cfg, host_st, PS.flat(rows), T, coeff_channels=cc, sst_in=sst, hdr=hdr, with_ps=with_ps)
    assert np.array_equal(host["taken"], got["taken"]) and np.array_equal(host["status"], got["status"])
    assert np.array_equal(PC.rows(host_st, S), PC.rows(after, S))
    return got, after, mdl


_POOLS = {}
AAC_CASES = [(False, 2, 3, 1), (False, 2, 3, 2), (True, 2, 3, 2), (True, 1, 4, 2)]      # mono cc 1 / 2, stereo LC, stereo Main


def pool(cpe, aot, si):
    """In-scope units of very different lengths, raw and behind ADTS headers, drawn once per configuration."""
    key = (cpe, aot, si)
    if key not in _POOLS:
        rng = np.random.default_rng(6000 + 7 * si + cpe + 100 * aot)
        _POOLS[key] = [au for row in PC.in_scope_steps(rng, si, aot, cpe, 160, 1, adts=0.3, sbr=0.3) for au in row]
    return _POOLS[key]


@pytest.mark.parametrize("S", SIZES)
def test_aac_kernel_against_the_chained_one_unit_calls(pkg, dev, S):
    """Every pairing of configuration and T over the five sizes; units of very different lengths share one wave."""
    rng = np.random.default_rng(6100 + S)
    for j, (cpe, aot, si, cc) in enumerate(AAC_CASES):
        T = TS[(SIZES.index(S) + j) % len(TS)]
        cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
        units = pool(cpe, aot, si)
        rows = [[units[int(k)] for k in rng.integers(0, len(units), S)] for _ in range(T)]
        st = np.zeros(S, pkg.AAC_STREAM_DT)
        st["window_sequence"] = rng.integers(0, 4, (S, 2))
        got, after, _ = run(pkg, dev, cfg, st, rows, cc)
        assert (got["taken"] == T).all() and not got["hold"].any(), (S, T, got["taken"])
        if S >= 63:
            sizes = [len(a) for a in rows[0]]
            assert max(sizes) > 4 * min(sizes)


class HeStreams:
    """S writer streams of one kind behind their first header, which the host parses."""

    def __init__(self, pkg, rng, S, cpe, ps_modes):
        self.pkg, self.S, self.cpe = pkg, S, cpe
        self.cfg = SD.he_cfg(pkg, cpe)
        self.with_ps, self.cc = not cpe, 2 if cpe else 1
        self.tab = pkg.SbrHeaderTable(256)
        self.st = np.zeros(S, pkg.AAC_STREAM_DT)
        self.sst = pkg.sbr_streams(S)
        self.writers = SD.make_writers(pkg, S, cpe, ps_modes)
        for _ in range(2):
            host = SD.host_parse(pkg, self.cfg, self.st, self.sst, self.tab, SD.he_units(rng, self.writers, cpe), self.cc, self.with_ps)
            assert not host["status"].any()


@pytest.mark.parametrize("S", SIZES)
def test_he_kernel_against_the_chained_one_unit_calls(pkg, dev, S):
    """HE mono with Parametric Stereo (20 and 34 bands) and HE stereo, every T over the sizes."""
    rng = np.random.default_rng(6200 + S)
    for j, (cpe, ps_modes) in enumerate([(False, "20"), (False, "34"), (True, None)]):
        T = TS[(SIZES.index(S) + j) % len(TS)]
        h = HeStreams(pkg, rng, S, cpe, ps_modes)
        rows = [SD.he_units(rng, h.writers, cpe, crc=bool(t & 1)) for t in range(T)]
        got, after, _ = run(pkg, dev, h.cfg, h.st, rows, h.cc, h.sst, h.tab.headers(), h.with_ps)
        assert (got["taken"] == T).all() and not got["hold"].any(), (S, T, got["taken"])
        assert (got["sbr"]["start"] == 1).all()
        if not cpe:
            assert (got["ps"]["start"] == 1).any()


@pytest.mark.parametrize("cpe,aot,si", [(False, 2, 3), (True, 1, 4)])
def test_aac_lanes_of_one_wave_stop_at_different_units(pkg, dev, cpe, aot, si):
    rng = np.random.default_rng(6300 + cpe)
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    T = 4
    plan = PS.stop_plan(rng, PS.AAC_STOPS, [0, 1, 2, T - 1], T, whole=6)
    S = len(plan)
    assert S <= 64
    rows = PC.in_scope_steps(rng, si, aot, cpe, S, T, adts=0.3, sbr=0.3)
    for s, (kind, t0) in enumerate(plan):
        if kind:
            rows[t0][s] = PS.aac_stop_unit(rng, si, aot, cpe, kind, rows[t0][s])
    st = np.zeros(S, pkg.AAC_STREAM_DT)
    got, after, _ = run(pkg, dev, cfg, st, rows, 2)
    assert [int(x) for x in got["taken"]] == [t0 for _, t0 in plan]
    PS.check_against_host(pkg, cfg, got, after, st, rows, 2)


@pytest.mark.parametrize("cpe", [False, True])
def test_he_lanes_of_one_wave_stop_at_different_units(pkg, dev, cpe):
    """The stopping units of neighbouring lanes sit at different t0, some at t0 >= 2: the second SBR walk of such a lane
    covers more than one unit while its neighbours walk on."""
    rng = np.random.default_rng(6400 + cpe)
    T = 4
    plan = PS.stop_plan(rng, PS.HE_STOPS, [0, 1, 2, T - 1], T, whole=4)
    plan = [(k or "plain", t0) for k, t0 in plan]
    S = len(plan)
    h = HeStreams(pkg, rng, S, cpe, "any")
    rows = [SD.mixed_units(rng, h.writers, cpe, [kind if t == t0 else "plain" for kind, t0 in plan]) for t in range(T)]
    hdr = h.tab.headers()
    got, after, mdl = run(pkg, dev, h.cfg, h.st, rows, h.cc, h.sst, hdr, h.with_ps)
    rewalked = 0
    for s, (kind, t0) in enumerate(plan):
        if kind == "flipped":
            assert int(got["taken"][s]) >= t0
            continue
        assert int(got["taken"][s]) == t0, (s, kind, got["taken"][s])
        rewalked += kind not in ("plain", "aac_refused") and t0 >= 2
    assert rewalked >= 6 and mdl["putback"] >= 12
    PS.check_against_host(pkg, h.cfg, got, after, h.st, rows, h.cc, h.sst, h.tab, h.with_ps)


def test_aac_bytes_to_pcm_with_the_parsers_own_hold_mask(pkg, oracle, dev):
    """bytes -> aac_parse_streams -> heaac_spectral_tools_streams_ex -> heaac_lc_decode_streams_ex, nothing passing through
    the host: the PCM of the taken frames, zero PCM of the held ones and every final state are those of the oracle
    driven by the host-parsed records of the taken units."""
    import torch
    rng = np.random.default_rng(6500)
    cfg = TP._cfg(pkg, 2, 3, 2)
    S, T = 65, 3
    rows = PC.in_scope_steps(rng, 3, 2, True, S, T, adts=0.3, sbr=0.3)
    stops = {3: 0, 20: 1, 21: 2, 64: 1}
    for s, t0 in stops.items():
        rows[t0][s] = PS.aac_stop_unit(rng, 3, 2, True, "pulse" if s != 20 else "empty", rows[t0][s])
    st = np.zeros(S, pkg.AAC_STREAM_DT)
    ref_state = np.zeros((S, 1024), np.float32)
    ref_rng = np.full(S, 0x1f2e3d4c, np.int32)
    ref_pcm = np.zeros((S, T, 1024, 2), np.int16)
    for t in range(T):
        idx = np.array([s for s in range(S) if stops.get(s, T) > t])
        sub = st[idx].copy()
        host = pkg.aac_parse_batch(cfg, sub, [rows[t][s] for s in idx])
        assert host["failed"] == 0
        st[idx] = sub
        c, ref_rng[idx] = oracle.spectral_tools_batch(2, host["coeffs"], host["tools"], rng=ref_rng[idx])
        ref_pcm[idx, t], ref_state[idx] = oracle.lc_decode_batch(2, c, host["ics"], ref_state[idx], oracle.PCM_S16)
    d_au, d_off = load(pkg, PS.flat(rows))
    d_st = pkg.to_device(np.zeros(S, pkg.AAC_STREAM_DT))
    d_rng = torch.full((S,), 0x1f2e3d4c, dtype=torch.int32, device="cuda")
    out = dev.aac_parse_streams(cfg, d_st, d_au, d_off, T)
    dev.spectral_tools_streams(2, out["coeffs"], out["tools"], T, rng=d_rng, hold=out["hold"])
    pcm, d_state = dev.lc_decode_streams(2, out["coeffs"], out["ics"], torch.zeros((S, 1024), device="cuda"), T,
                                         pcm_format=pkg.PCM_S16, hold=out["hold"])
    torch.cuda.synchronize()
    assert [int(x) for x in out["taken"].cpu().numpy()] == [stops.get(s, T) for s in range(S)]
    got = pcm.cpu().numpy().reshape(S, T, 1024, 2)
    assert np.array_equal(got, ref_pcm)
    for s, t0 in stops.items():
        assert not got[s, t0:].any()
    assert np.abs(got).max() > 0
    assert np.array_equal(d_state.cpu().numpy().view(np.uint32), ref_state.view(np.uint32))
    assert np.array_equal(d_rng.cpu().numpy(), ref_rng)
    assert np.array_equal(PC.rows(d_st.cpu().numpy(), S), PC.rows(st, S))


def test_hev2_bytes_to_pcm_with_the_parsers_own_hold_mask(pkg, oracle, dev):
    """The same for HE-AACv2 through heaac_he_decode_streams_ex (S = 8, T = 3; one stream stops at a new header)."""
    import torch
    rng = np.random.default_rng(6600)
    S, T, hcfg = 8, 3, pkg.CFG_HEV2
    h = HeStreams(pkg, rng, S, False, "any")
    stops = {2: 1, 5: 2}
    rows = [SD.mixed_units(rng, h.writers, False, ["new_header" if stops.get(s) == t else "plain" for s in range(S)]) for t in range(T)]
    hdr = h.tab.headers()
    d_hdr = pkg.to_device(hdr)
    st, sst = h.st.copy(), h.sst.copy()
    ref_state = np.zeros((S, pkg.STATE_WORDS[hcfg]), np.float32)
    ref_rng = np.full(S, 0x1f2e3d4c, np.int32)
    ref_pcm = np.zeros((S, T, 2, 2048), np.float32)
    scale = np.ones((S, T), np.float32)
    for t in range(T):
        idx = np.array([s for s in range(S) if stops.get(s, T) > t])
        a, b = st[idx].copy(), sst[idx].copy()
        host = pkg.heaac_parse_batch(h.cfg, a, b, h.tab, [rows[t][s] for s in idx], with_ps=True)
        assert host["failed"] == 0 and len(h.tab) == len(hdr)
        st[idx], sst[idx] = a, b
        c, ref_rng[idx] = oracle.spectral_tools_batch(1, np.ascontiguousarray(host["coeffs"][:, :1]), host["tools"], rng=ref_rng[idx])
        # (the writer's escape values reach far beyond full scale: down by a power of two, exact on both sides)
        scale[idx, t] = 2.0 ** -np.ceil(np.log2(np.maximum(np.abs(c).max(axis=(1, 2)), 1.0)))
        ref_pcm[idx, t], ref_state[idx] = oracle.he_decode_batch(hcfg, c * scale[idx, t][:, None, None], np.ascontiguousarray(host["ics"][:, :1]),
                                                                 host["sbr"], hdr, host["ps"], ref_state[idx], pkg.PCM_F32)
    d_au, d_off = load(pkg, PS.flat(rows))
    d_st = pkg.to_device(h.st.copy())
    d_rng = torch.full((S,), 0x1f2e3d4c, dtype=torch.int32, device="cuda")
    out = dev.heaac_parse_device_streams(h.cfg, d_st, pkg.to_device(h.sst), d_au, d_off, d_hdr, T, coeff_channels=1)
    dev.spectral_tools_streams(1, out["coeffs"], out["tools"], T, rng=d_rng, hold=out["hold"])
    out["coeffs"].mul_(torch.from_numpy(scale.reshape(-1)).cuda()[:, None, None])
    pcm, d_state = dev.he_decode_streams(hcfg, out["coeffs"], out["ics"], out["sbr"], d_hdr, out["ps"],
                                         torch.zeros((S, pkg.STATE_WORDS[hcfg]), device="cuda"), T, hold=out["hold"])
    torch.cuda.synchronize()
    assert [int(x) for x in out["taken"].cpu().numpy()] == [stops.get(s, T) for s in range(S)]
    got = pcm.cpu().numpy().reshape(S, T, 2, 2048)
    assert np.isfinite(ref_pcm).all() and np.abs(ref_pcm).max() > 0
    assert np.array_equal(got.view(np.uint32), ref_pcm.view(np.uint32))
    for s, t0 in stops.items():
        assert not got[s, t0:].any()
    assert np.array_equal(d_state.cpu().numpy().view(np.uint32), ref_state.view(np.uint32))
    assert np.array_equal(d_rng.cpu().numpy(), ref_rng)
    assert np.array_equal(PC.rows(d_st.cpu().numpy(), S), PC.rows(st, S))
    assert np.array_equal(out["sst"].cpu().numpy().reshape(S, -1), sst)


def test_captured_into_a_graph_and_replayed_with_fresh_bytes(pkg, dev):
    """The HE call is a prep kernel and the walk on the caller's stream: captured once, replayed with other bytes in the
    same buffers (every record 0xA5-refilled), it gives the records of those bytes -- the prep kernel's zeroes included."""
    import torch
    rng = np.random.default_rng(6700)
    S, T = 100, 3
    h = HeStreams(pkg, rng, S, False, "any")
    keep = [SD.snapshot(w) for w in h.writers]
    first = [SD.he_units(rng, h.writers, False) for _ in range(T)]
    # other bytes from the same states: no payload / a repeated header in mid-chain, and a new header that stops every
    # fifth stream at its second unit
    for w, k in zip(h.writers, keep):
        SD.restore(w, k)
    second = []
    for t in range(T):
        classes = [("new_header" if s % 5 == 0 else "no_payload" if s % 2 else "same_header") if t == 1 else "plain" for s in range(S)]
        second.append(SD.mixed_units(rng, h.writers, False, classes))
    hdr = h.tab.headers()
    d_hdr = pkg.to_device(hdr)
    n, cap = S * T, S * T * 1500
    d_au = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    d_st = pkg.to_device(h.st.copy())
    d_in = pkg.to_device(h.sst)
    pre = PS.filled_streams(pkg, S, T, 1, h.sst, True)
    pre.pop("why")
    pre["taken"] = pre["taken"].view(np.int32)
    d = {k: pkg.to_device(v) for k, v in pre.items()}

    def fill(rows):
        buf, off = pkg.pack_units(PS.flat(rows))
        assert buf.size <= cap
        d_au[:buf.size].copy_(torch.from_numpy(buf))
        d_off.copy_(torch.from_numpy(off.astype(np.int32)))
        d_st.copy_(pkg.to_device(h.st.copy()))
        for v in d.values():
            v.view(torch.uint8).fill_(FILL)

    def call():
        dev.heaac_parse_device_streams(h.cfg, d_st, d_in, d_au, d_off, d_hdr, T, coeff_channels=1, coeffs=d["coeffs"].view(-1),
                                       ics=d["ics"], tools=d["tools"], info=d["info"], sst_out=d["sst"].view(-1), sbr=d["sbr"],
                                       ps=d["ps"], status=d["status"], taken=d["taken"], hold=d["hold"])

    def records():
        torch.cuda.synchronize()
        got = dict(coeffs=d["coeffs"].cpu().numpy(), ics=d["ics"].cpu().numpy().view(pkg.ICS_DT).reshape(n, 1),
                   tools=d["tools"].cpu().numpy().view(pkg.TOOLS_FRAME_DT), info=d["info"].cpu().numpy().view(pkg.AAC_INFO_DT),
                   status=d["status"].cpu().numpy(), taken=d["taken"].cpu().numpy().view(np.uint32), hold=d["hold"].cpu().numpy(),
                   sst=d["sst"].cpu().numpy().reshape(S, -1), sbr=d["sbr"].cpu().numpy().view(pkg.SBR_FRAME_DT),
                   ps=d["ps"].cpu().numpy().view(pkg.PS_FRAME_DT))
        return got, d_st.cpu().numpy().view(pkg.AAC_STREAM_DT)

    s = torch.cuda.Stream()
    fill(first)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()                                         # warm-up on the capture stream
    torch.cuda.synchronize()
    fill(first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    for rows in (first, second):
        fill(rows)
        torch.cuda.synchronize()
        g.replay()
        got, after = records()
        host_st = h.st.copy()
        host = pkg.parse_core_streams(h.cfg, host_st, PS.flat(rows), T, coeff_channels=1, sst_in=h.sst, hdr=hdr, with_ps=True,
                                      out=PS.filled_streams(pkg, S, T, 1, h.sst, True))
        host.update(st=host_st, putback=0)
        PS.compare_with_model(pkg, got, after, host, S, T)
        # the tools, sbr and ps records whole: what only the prep kernel writes (the zeroes) is there on replay
        ok = got["status"] == 0
        for k in ("tools", "sbr", "ps"):
            assert np.array_equal(PC.rows(got[k], n)[ok], PC.rows(host[k], n)[ok]), k
        assert ok.all() if rows is first else ((got["taken"][::5] == 1).all() and (np.delete(got["taken"], np.s_[::5]) == T).all())


def test_device_entries_refuse_bad_arguments_before_any_launch(pkg, dev):
    """Both entries with a real device: every array NULL in turn, T == 0, overlapping state arrays, misaligned pointers,
    n_hdr == 0, coeff_channels 0 / 3 and an S * T beyond the unit index are HEAAC_ERR_ARG and leave the canary in every
    output; S == 0 is HEAAC_OK; and the same arguments as they should be parse."""
    import torch
    f = pkg.lib().heaac_aac_parse_device_streams
    g = pkg.lib().heaac_heaac_parse_device_streams
    rng = np.random.default_rng(6800)
    S, T = 4, 2
    h = HeStreams(pkg, rng, S, False, "any")
    rows = [SD.he_units(rng, h.writers, False) for _ in range(T)]
    d_au, d_off = load(pkg, PS.flat(rows))
    d_hdr = pkg.to_device(h.tab.headers())
    d_in = pkg.to_device(h.sst)
    pre = PS.filled_streams(pkg, S, T, 1, h.sst, True)
    pre.pop("why")
    pre["taken"] = pre["taken"].view(np.int32)
    d = {k: pkg.to_device(v) for k, v in pre.items()}
    d_st = torch.full((S * pkg.AAC_STREAM_DT.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    P = lambda k: d[k].data_ptr()
    good_f = [dev._h, C.addressof(h.cfg), d_st.data_ptr(), d_au.data_ptr(), d_off.data_ptr(), S, T, 1, P("coeffs"), P("ics"), P("tools"),
              P("info"), P("status"), P("taken"), P("hold"), None]
    good_g = good_f[:3] + [d_in.data_ptr(), P("sst")] + good_f[3:12] + [d_hdr.data_ptr(), len(h.tab), P("sbr"), P("ps")] + good_f[12:]
    row = h.sst.shape[1]

    def untouched():
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == FILL).all()
        for k, v in d.items():
            assert (v.cpu().numpy().reshape(-1).view(np.uint8) == FILL).all(), k

    def refused(fn, good, k, v):
        bad = list(good)
        bad[k] = v
        assert fn(*bad) == -1, (fn is g, k, v)

    for k in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13):
        refused(f, good_f, k, None)
    for k in (0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 16, 17, 18, 19):
        refused(g, good_g, k, None)
    for fn, good, at in ((f, good_f, 5), (g, good_g, 7)):
        refused(fn, good, at + 1, 0)                                   # T == 0
        refused(fn, good, at + 2, 0)
        refused(fn, good, at + 2, 3)
        refused(fn, good, at, 1 << 31)                                 # S * T beyond the 32-bit unit index
        refused(fn, good, at, (1 << 63) + 1)                           # S * T overflows
    for k in (4, 8, 10, 11, 12, 13):
        refused(f, good_f, k, good_f[k] + 2)
    for k in (3, 4, 6, 10, 12, 13, 14, 16, 18, 19):
        refused(g, good_g, k, good_g[k] + 2)
    refused(g, good_g, 15, 0)                                          # n_hdr == 0
    refused(g, good_g, 3, P("sst"))                                    # the state arrays are the same, or overlap
    refused(g, good_g, 3, P("sst") + row)
    refused(g, good_g, 4, d_in.data_ptr() + 2 * row)
    untouched()
    for fn, good, at in ((f, good_f, 5), (g, good_g, 7)):
        zero = list(good)
        zero[at] = 0
        assert fn(*zero) == 0
        for k in range(2, len(zero) - 1):
            if k not in (at, at + 1, at + 2):
                zero[k] = None if not (fn is g and k == 15) else 0
        assert fn(*zero) == 0
    untouched()
    d_st.copy_(pkg.to_device(h.st.copy()))
    assert g(*good_g) == 0
    torch.cuda.synchronize()
    assert not d["status"].cpu().numpy().any() and (d["taken"].cpu().numpy().view(np.uint32) == T).all() and not d["hold"].cpu().numpy().any()
    d_st.copy_(pkg.to_device(h.st.copy()))
    assert f(*good_f) == 0
    torch.cuda.synchronize()
    assert not d["status"].cpu().numpy().any()
