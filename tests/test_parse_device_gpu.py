"""heaac_aac_parse_device on the GPU against the host parser heaac_aac_parse_frame_ex: the corpora and the assertions of
test_parse_core.py through the kernel (one lane per unit), every output pre-filled with a NaN pattern on both sides,
the composed chain bytes -> parse -> tools -> decode against the oracle, and the call captured into a graph.

Kernel and host parser read the element syntax through the same pc_* readers of csrc/parse_core.h: what is pinned
here is the device against the host (the compiler's device code, the LDS copy of the prefix tables, the fill kernel,
the defer mode against the host's refuse mode), not one writing of the syntax against another."""
import numpy as np
import pytest

import parse_device_common as PC
import test_parse as TP

pytestmark = pytest.mark.gpu
NAN = 0xFF                       # float32 0xffffffff: a NaN no parser writes


def device_parse(pkg, dev, cfg, st, aus, cc):
    """One call on the GPU from the states `st` (numpy AAC_STREAM_DT, left alone) with every output NaN-filled.
    Returns (records as numpy arrays, the states after the call)."""
    import torch
    n = len(aus)
    buf, off = pkg.pack_units(aus)
    d_au = torch.from_numpy(np.concatenate([buf, np.zeros(1, np.uint8)])).cuda()[:buf.size]
    d_st = pkg.to_device(st.copy())
    pre = {k: pkg.to_device(v) for k, v in PC.filled(pkg, n, cc, NAN).items()}
    d_status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    out = dev.aac_parse(cfg, d_st, d_au, off, coeff_channels=cc, coeffs=pre["coeffs"], ics=pre["ics"], tools=pre["tools"],
                        info=pre["info"], status=d_status)
    torch.cuda.synchronize()
    got = dict(coeffs=out["coeffs"].cpu().numpy(), ics=out["ics"].cpu().numpy().view(pkg.ICS_DT).reshape(n, cc),
               tools=out["tools"].cpu().numpy().view(pkg.TOOLS_FRAME_DT), info=out["info"].cpu().numpy().view(pkg.AAC_INFO_DT),
               status=out["status"].cpu().numpy())
    return got, d_st.cpu().numpy().view(pkg.AAC_STREAM_DT)


def run(pkg, dev, cfg, st, aus, cc):
    got, after = device_parse(pkg, dev, cfg, st, aus, cc)
    host, ok = PC.compare(pkg, cfg, st, aus, cc, got, after, fill=NAN)
    return host, ok, got, after


@pytest.mark.parametrize("cpe,aot,si", [(False, 2, 3), (True, 2, 3), (True, 1, 4), (False, 2, 6), (True, 2, 11), (False, 1, 4)])
def test_in_scope_units_on_the_gpu(pkg, dev, cpe, aot, si):
    """n = 1, 63, 64, 65 and a few thousand; units of very different lengths in one wave (max_sfb 1 .. all bands,
    SBR payloads, ADTS headers); chained so that the window history and the tag / configuration state matter."""
    rng = np.random.default_rng(8800 + 7 * si + cpe + 100 * aot)
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    pool = [au for row in PC.in_scope_steps(rng, si, aot, cpe, 200, 1, adts=0.3, sbr=0.3) for au in row]
    for cc in ((2,) if cpe else (1, 2)):
        for n in (1, 63, 64, 65, 3000):
            st = np.zeros(n, pkg.AAC_STREAM_DT)
            for step in range(2):
                if n <= 65:
                    aus = PC.in_scope_steps(rng, si, aot, cpe, n, 1, adts=0.3, sbr=0.3)[0]
                else:
                    # (raw and ADTS-framed units may follow each other in one stream: the tag state must follow)
                    aus = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
                sizes = [len(a) for a in aus]
                host, ok, got, st = run(pkg, dev, cfg, st, aus, cc)
                assert not host.any(), ("precondition: the host parser takes the whole corpus", np.flatnonzero(host)[:8])
                assert ok.all(), ("deferred in-scope units", n, step, np.flatnonzero(~ok)[:8])
                if n >= 63:
                    assert max(sizes) > 4 * min(sizes)


@pytest.mark.parametrize("cpe,aot,si", [(False, 2, 3), (True, 2, 3), (True, 1, 4)])
def test_deferred_and_damaged_units_on_the_gpu(pkg, dev, cpe, aot, si):
    """The deferred classes and the damage, mixed with good units in the same waves: the kernel's verdicts are the
    host walk's (heaac_debug_aac_parse_core), unit for unit, and PC.compare's rules hold against the host parser."""
    rng = np.random.default_rng(9900 + cpe + aot)
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    good = [au for row in PC.in_scope_steps(rng, si, aot, cpe, 40, 1, adts=0.4, sbr=0.3) for au in row]
    deferred = PC.deferred_units(rng, si, aot, cpe, 16)
    aus = good + deferred + PC.damaged_units(rng, good[:8] + deferred[:4]) + PC.written_refusals(rng, si, aot, cpe)
    order = rng.permutation(len(aus))
    aus = [aus[int(k)] for k in order]
    st = np.zeros(len(aus), pkg.AAC_STREAM_DT)
    st["window_sequence"] = rng.integers(0, 4, (len(aus), 2))
    st["mapped_tag"] = rng.integers(0, 2, len(aus))
    st["oc"] = rng.choice([0, 1, 2, 4, 8, 12], len(aus))
    for cc in ((2,) if cpe else (1, 2)):
        host, ok, got, after = run(pkg, dev, cfg, st, aus, cc)
        core_st = st.copy()
        core = pkg.aac_parse_core(cfg, core_st, aus, coeff_channels=cc, out=PC.filled(pkg, len(aus), cc, NAN))
        assert np.array_equal(core["status"], got["status"]), np.flatnonzero(core["status"] != got["status"])[:8]
        assert np.array_equal(PC.rows(core_st, len(aus)), PC.rows(after, len(aus)))
        was_deferred = np.isin(order, np.arange(len(good), len(good) + len(deferred)))
        assert not ok[was_deferred].any() and ok[order < len(good)].all()
        wrongly = (host == 0) & ~ok & (core["why"] == pkg.PARSE_WHY_REFUSED)
        assert not wrongly.any(), np.flatnonzero(wrongly)[:8]
        assert ok.sum() > 60 and (host != 0).sum() > 200


def test_main_profile_tns_up_to_order_20_on_the_gpu(pkg, dev):
    rng = np.random.default_rng(2021)
    cfg = TP._cfg(pkg, 1, 4, 1)
    units = PC.main_high_order_units(rng, 4, 80)
    aus = [u for u, _ in units]
    for cc in (1, 2):
        host, ok, got, _ = run(pkg, dev, cfg, np.zeros(len(aus), pkg.AAC_STREAM_DT), aus, cc)
        assert not host.any() and ok.all()
        assert [int(t["ch"][0]["tns"]["order"][0][0]) for t in got["tools"]] == [o for _, o in units]


def test_device_entry_refuses_bad_arguments_before_any_launch(pkg, dev):
    """heaac_aac_parse_device itself, with a real device: every array NULL in turn, a d_coeffs that is not 16-byte
    aligned, coeff_channels / sampling_index / object type out of range are HEAAC_ERR_ARG and write nothing; n = 0 is
    HEAAC_OK whatever the arrays are."""
    import ctypes as C
    import torch
    f = pkg.lib().heaac_aac_parse_device
    n = 4
    aus = PC.in_scope_steps(np.random.default_rng(5), 3, 2, True, n, 1)[0]
    buf, off = pkg.pack_units(aus)
    d_au = torch.from_numpy(buf).cuda()
    d_off = torch.from_numpy(off.astype(np.int32)).cuda()
    d_st = torch.zeros(n * pkg.AAC_STREAM_DT.itemsize, dtype=torch.uint8, device="cuda")
    pre = {k: pkg.to_device(v) for k, v in PC.filled(pkg, n, 2, NAN).items()}
    d_status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    d_spare = torch.zeros(n * 2 * 1024 + 4, dtype=torch.float32, device="cuda")
    cfg = TP._cfg(pkg, 2, 3, 2)
    good = [dev._h, C.addressof(cfg), d_st.data_ptr(), d_au.data_ptr(), d_off.data_ptr(), n, 2, pre["coeffs"].data_ptr(),
            pre["ics"].data_ptr(), pre["tools"].data_ptr(), pre["info"].data_ptr(), d_status.data_ptr(), None]

    def untouched():
        torch.cuda.synchronize()
        assert (d_status.cpu().numpy() == 7).all() and not d_st.cpu().numpy().any()
        for v in pre.values():
            assert (v.cpu().numpy().reshape(-1).view(np.uint8) == NAN).all()

    for k in (0, 1, 2, 3, 4, 7, 8, 9, 10, 11):
        bad = list(good)
        bad[k] = None
        assert f(*bad) == -1, k
    bad = list(good)
    bad[7] = d_spare.data_ptr() + 4                       # 4-byte aligned, not 16
    assert f(*bad) == -1
    for cc in (0, 3, -1):
        bad = list(good)
        bad[6] = cc
        assert f(*bad) == -1, cc
    for field, value in (("sampling_index", 13), ("sampling_index", -1), ("object_type", 5), ("object_type", 0)):
        c = TP._cfg(pkg, 2, 3, 2)
        setattr(c, field, value)
        bad = list(good)
        bad[1] = C.addressof(c)
        assert f(*bad) == -1, (field, value)
    untouched()
    zero = list(good)
    zero[5] = 0
    assert f(*zero) == 0
    for k in (2, 3, 4, 7, 8, 9, 10, 11):
        zero[k] = None
    assert f(*zero) == 0
    untouched()
    assert f(*good) == 0                                  # and the same arguments as they should be parse
    torch.cuda.synchronize()
    assert not d_status.cpu().numpy().any()


def test_bytes_to_pcm_on_one_stream(pkg, oracle, dev):
    """bytes -> heaac_aac_parse_device -> heaac_spectral_tools_batch -> heaac_lc_decode_batch with nothing passing
    through the host, three chained frames: the PCM and every state the host-parsed records give through the oracle
    (the comparison of test_parse.py::test_bitstream_to_pcm_on_the_gpu)."""
    import torch
    rng = np.random.default_rng(77)
    cfg = TP._cfg(pkg, 2, 3, 2)
    n = 48
    st = np.zeros(n, pkg.AAC_STREAM_DT)
    d_st = pkg.to_device(st.copy())
    d_state = torch.zeros((n, 1024), device="cuda")
    ref_state = np.zeros((n, 1024), np.float32)
    d_rng = torch.full((n,), 0x1f2e3d4c, dtype=torch.int32, device="cuda")
    ref_rng = np.full(n, 0x1f2e3d4c, np.int32)
    for step, aus in enumerate(PC.in_scope_steps(rng, 3, 2, True, n, 3, adts=0.3, sbr=0.3)):
        host = pkg.aac_parse_batch(cfg, st, aus)
        assert host["failed"] == 0
        ref_c, ref_rng = oracle.spectral_tools_batch(2, host["coeffs"], host["tools"], rng=ref_rng)
        ref_pcm, ref_state = oracle.lc_decode_batch(2, ref_c, host["ics"], ref_state, oracle.PCM_S16)
        buf, off = pkg.pack_units(aus)
        out = dev.aac_parse(cfg, d_st, torch.from_numpy(buf).cuda(), off)
        dev.spectral_tools(2, out["coeffs"], out["tools"], rng=d_rng)
        pcm, d_state = dev.lc_decode(2, out["coeffs"], out["ics"], d_state, pcm_format=pkg.PCM_S16)
        assert not out["status"].cpu().numpy().any(), step
        assert np.array_equal(out["coeffs"].cpu().numpy().view(np.uint32), ref_c.view(np.uint32)), step
        assert np.array_equal(pcm.cpu().numpy(), ref_pcm), step
        assert np.array_equal(d_state.cpu().numpy().view(np.uint32), ref_state.view(np.uint32)), step
        assert np.array_equal(d_rng.cpu().numpy(), ref_rng), step
        assert np.array_equal(PC.rows(d_st.cpu().numpy(), n), PC.rows(st, n)), step


def test_captured_into_a_graph_and_replayed_with_fresh_bytes(pkg, dev):
    """The call is a fill and one kernel on the caller's stream: captured once (a linear graph), replayed with other
    bytes in the same buffers, it gives the records of those bytes."""
    import torch
    rng = np.random.default_rng(123)
    cfg = TP._cfg(pkg, 2, 3, 2)
    n, cap = 200, 200 * 1200
    first, second = PC.in_scope_steps(rng, 3, 2, True, n, 2, adts=0.3, sbr=0.3)
    d_au = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    d_st = torch.zeros(n * pkg.AAC_STREAM_DT.itemsize, dtype=torch.uint8, device="cuda")
    pre = {k: pkg.to_device(v) for k, v in PC.filled(pkg, n, 2, NAN).items()}
    d_status = torch.full((n,), 7, dtype=torch.int32, device="cuda")

    def load(aus):
        buf, off = pkg.pack_units(aus)
        assert buf.size <= cap
        d_au[:buf.size].copy_(torch.from_numpy(buf))
        d_off.copy_(torch.from_numpy(off.astype(np.int32)))
        d_st.zero_()
        for v in pre.values():
            v.fill_(NAN) if v.dtype == torch.uint8 else v.view(torch.int32).fill_(-1)

    def call():
        dev.aac_parse(cfg, d_st, d_au, d_off, coeff_channels=2, coeffs=pre["coeffs"], ics=pre["ics"], tools=pre["tools"],
                      info=pre["info"], status=d_status)

    def records():
        torch.cuda.synchronize()
        got = dict(coeffs=pre["coeffs"].cpu().numpy(), ics=pre["ics"].cpu().numpy().view(pkg.ICS_DT).reshape(n, 2),
                   tools=pre["tools"].cpu().numpy().view(pkg.TOOLS_FRAME_DT), info=pre["info"].cpu().numpy().view(pkg.AAC_INFO_DT),
                   status=d_status.cpu().numpy())
        return got, d_st.cpu().numpy().view(pkg.AAC_STREAM_DT)

    s = torch.cuda.Stream()
    load(first)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()                                         # warm-up on the capture stream
    torch.cuda.synchronize()
    load(first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    zero = np.zeros(n, pkg.AAC_STREAM_DT)
    for aus in (first, second):
        load(aus)
        torch.cuda.synchronize()
        g.replay()
        got, after = records()
        host, ok = PC.compare(pkg, cfg, zero, aus, 2, got, after, fill=NAN)
        assert not host.any() and ok.all()
