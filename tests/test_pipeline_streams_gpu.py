"""The pipeline's streams form (heaac_pipeline_create_streams: T access units per stream and tick, the streams calls with
hold masks on the GPU) against the same pipeline at one unit per tick: Pipeline(..., frames_per_tick=1), fed the same
units over K * T ticks.  PCM and status bit for bit: T units in one tick = T ticks of one unit; later ticks depend on
the state carried across the tick boundary, so the state is covered through the PCM.  Both sides are one code path (a
one-unit tick is held by the same masks), so the one-unit pipeline is itself compared, on the damaged corpus, with
something that shares no code with it: one heaac_codec_decode context per stream (csrc/shim.hip), which refuses a
damaged unit before it touches the DSP -- no mask, nothing to hold."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest

import refused_units as RU
import sbr_bitwriter as SW
import test_parse as TP
import test_sbr_parse as TS

pytestmark = pytest.mark.gpu

K = 3                    # ticks, all submitted before the first collect (K <= HEAAC_PIPELINE_DEPTH)
T_MAX = 8
TS_PER_TICK = [2, 5, 8]
CASES = ["hev2", "hev1", "hev1_down", "lc_stereo_main", "lc_mono"]
OURS_ONLY = bytes([0x40, 0]) + bytes(8)      # a coupling element in a one-element stream: only this parser refuses it
                                             # (tests/test_pipeline.py)

_units = {}


def _case(pkg, name):
    """(AacConfig, he_cfg, n, units[n][K * T_MAX], si, aot, element): the streams' units are drawn once per case"""
    if name.startswith("hev"):
        ps = name == "hev2"
        channels = 1 if ps else 2
        m4 = TS._he_cfg(pkg, channels, ps)
        if name == "hev1_down":                      # extension rate = core rate: 1024 samples per unit
            m4.ext_sampling_index, m4.ext_sample_rate = m4.sampling_index, m4.sample_rate
        cfg, n, si, aot = (pkg.CFG_HEV2 if ps else pkg.CFG_HEV1), 7, 6, 2
    elif name == "lc_stereo_main":
        m4, cfg, n, si, aot, channels = TP._cfg(pkg, 1, 3, 2), pkg.CFG_LC_STEREO, 7, 3, 1, 2
    else:
        m4, cfg, n, si, aot, channels = TP._cfg(pkg, 2, 3, 1), pkg.CFG_LC_MONO, 7, 3, 2, 1      # n odd
    if name not in _units:
        rng = np.random.default_rng(900 + CASES.index(name))
        total = K * T_MAX
        if name.startswith("hev"):
            writers = [SW.SbrStreamWriter(pkg, channels, ps=ps, ps_modes="20" if ps else "any") for _ in range(n)]
            per = [[] for _ in range(n)]
            for u in range(total):
                for i, w in enumerate(writers):
                    while True:                      # (as tests/test_pipeline.py: a payload that fits its fill element)
                        keep = copy.deepcopy((w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling))
                        bits, _ = w.frame(rng, new_header=(u == 3))
                        if (4 + len(bits) + 7) // 8 <= 269:
                            break
                        w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling = keep
                    per[i].append(TP._write_au(rng, si, aot, channels == 2, extras=False, sbr=(bits, False), quiet=True)[0])
        else:
            per = [[TP._write_au(rng, si, aot, channels == 2, extras=True, quiet=True)[0] for _ in range(total)]
                   for _ in range(n)]
        _units[name] = per
    return m4, cfg, n, _units[name], si, aot, channels


def _reference(pkg, m4, cfg, n, units, total):
    """the one-unit-per-tick pipeline over `total` ticks: PCM [total][n][len][ch], status [total][n]"""
    pl = pkg.Pipeline(m4, cfg, n, threads=2, frames_per_tick=1)
    pcm, status = [], []
    for u in range(total):
        status.append(np.array(pl.submit([units[i][u] for i in range(n)])).copy())
        pcm.append(pl.collect().copy())
    pl.close()
    return np.stack(pcm), np.stack(status)


def _streams(pkg, m4, cfg, n, units, T, threads):
    """K ticks of T units per stream, all submitted before the first collect: PCM [K][n][T][len][ch], status [K][n][T]"""
    pl = pkg.Pipeline(m4, cfg, n, threads=threads, frames_per_tick=T)
    status = []
    for k in range(K):
        status.append(np.array(pl.submit([units[i][k * T + t] for i in range(n) for t in range(T)])).copy().reshape(n, T))
    pcm = [pl.collect().copy() for _ in range(K)]
    with pytest.raises(pkg.HeaacError):
        pl.collect()                                  # nothing in flight
    tm = pl.timing()
    assert tm["parse"] > 0 and tm["gpu"] > 0
    pl.close()
    return np.stack(pcm), np.stack(status)


def _compare(got, status, ref, ref_status, n, T):
    assert got.shape == (K, n, T) + ref.shape[2:], (got.shape, ref.shape)
    for k in range(K):
        for t in range(T):
            assert np.array_equal(status[k][:, t], ref_status[k * T + t]), ("status", k, t)
            same = (got[k][:, t] == ref[k * T + t]).reshape(n, -1).all(axis=1)
            assert same.all(), ("PCM", k, t, "streams", np.nonzero(~same)[0].tolist())


@pytest.mark.parametrize("T", TS_PER_TICK)
@pytest.mark.parametrize("name", CASES)
def test_streams_ticks_equal_one_unit_ticks(pkg, dev, name, T):
    m4, cfg, n, units, *_ = _case(pkg, name)
    ref, ref_status = _reference(pkg, m4, cfg, n, units, K * T)
    assert (ref_status >= 0).all()
    assert int(np.abs(ref.astype(int)).max()) > 50
    got, status = _streams(pkg, m4, cfg, n, units, T, threads=2)
    _compare(got, status, ref, ref_status, n, T)


def _damage(pkg, name, T):
    """units[n][K * T] with damaged ones; returns (units, {stream: [damaged unit indices]}, the damaged units)"""
    m4, cfg, n, clean, si, aot, channels = _case(pkg, name)
    rng = np.random.default_rng(77 + T)
    kinds = RU.KINDS_CPE if channels == 2 else RU.KINDS_SCE
    writer = RU.cpe_unit if channels == 2 else RU.sce_unit
    pool = itertools.cycle([None] + [k for k in kinds])          # None: the unit only this parser refuses
    units = [list(u[:K * T]) for u in clean]
    where = {0: [T],                                             # position 0 (of tick 1)
             1: [T // 2],                                        # the middle (of tick 0)
             2: [2 * T - 1],                                     # last (of tick 1)
             3: [T - 1, T] + ([2 * T - 3, 2 * T - 2] if T >= 5 else []),   # two in a row: across the tick boundary, inside a tick
             4: list(range(T, 2 * T))}                           # a whole tick of one stream
    damaged = []
    for s, us in where.items():
        for u in us:
            kind = next(pool)
            units[s][u] = OURS_ONLY if kind is None else writer(rng, si, aot, kind)[0]
            damaged.append(units[s][u])
    # a stream that has run out of units for the rest of tick 1 (and comes back in tick 2)
    where[5] = list(range(T + 1, 2 * T))
    for u in where[5]:
        units[5][u] = b""
    return m4, cfg, n, units, where, damaged


def _both_refusal_kinds_occur(pkg, name, m4, damaged):
    """on the CPU, with the host parser: every damaged unit fails in its core element; at least one asks for the tools
    to run all the same (HEAAC_REFUSED_RUN_TOOLS) and at least one does not"""
    k = len(damaged)
    st = np.zeros(k, pkg.AAC_STREAM_DT)
    if name.startswith("hev"):
        tab = pkg.SbrHeaderTable(64)
        q = pkg.heaac_parse_batch(m4, st, pkg.sbr_streams(k), tab, damaged, threads=1, with_ps=name == "hev2")
        tab.close()
    else:
        q = pkg.aac_parse_batch(m4, st, damaged, threads=1)
    assert (q["status"] < 0).all() and (q["info"]["channels"] == 0).all()
    run = (q["info"]["refused"] & pkg.REFUSED_RUN_TOOLS) != 0
    assert run.any() and (~run).any(), q["info"]["refused"].tolist()


@pytest.mark.parametrize("T", TS_PER_TICK)
@pytest.mark.parametrize("name", CASES)
def test_damaged_units_in_streams_ticks(pkg, dev, name, T):
    m4, cfg, n, units, where, damaged = _damage(pkg, name, T)
    _both_refusal_kinds_occur(pkg, name, m4, damaged)
    ref, ref_status = _reference(pkg, m4, cfg, n, units, K * T)
    for s, us in where.items():
        for u in us:
            assert ref_status[u][s] < 0 and not ref[u][s].any(), (s, u)
        # silence against silence would show nothing: the stream is heard again after its damaged units
        assert ref[max(us) + 1:, s].any(), s
    assert (ref_status[:, 6] >= 0).all()
    results = []
    for threads in (1, 2):
        got, status = _streams(pkg, m4, cfg, n, units, T, threads)
        _compare(got, status, ref, ref_status, n, T)
        results.append(got)
    assert np.array_equal(results[0], results[1])


# The configurations of the cases as a codec context takes them (AudioSpecificConfig: tests/test_pipeline_vs_codec_gpu.py,
# tests/test_shim_gpu.py), with the samples and channels of one decoded unit.  The AAC-LC / Main ones end in the sync
# extension 0x2b7 with sbrPresentFlag = 0: _case() writes their units with extras, some of which carry a fill element
# of SBR type, and a context left to implicit signalling would turn SBR on at the first of them; TP._cfg (sbr = 0)
# tells the pipeline explicitly that there is none.
def _lc_asc(aot, ch):
    return bytes([(aot << 3) | 1, 0x80 | (ch << 3), 0x56, 0xE5, 0x00])


CODEC = {"hev2": (bytes([0xEB, 0x09, 0x88, 0x00]), 2048, 2), "hev1": (bytes([0x2B, 0x11, 0x88, 0x00]), 2048, 2),
         "hev1_down": (bytes([0x2B, 0x13, 0x08, 0x00]), 1024, 2), "lc_stereo_main": (_lc_asc(1, 2), 1024, 2),
         "lc_mono": (_lc_asc(2, 1), 1024, 1)}


@pytest.mark.parametrize("name", CASES)
def test_one_unit_ticks_equal_codec_contexts_on_damaged_units(pkg, dev, name):
    """The reference of the tests above, anchored: the damaged corpus of T = 5 through the one-unit pipeline and through
    one codec context per stream, unit for unit -- refused there <=> negative status and silence here, otherwise the
    same PCM.  Stream 5 is left out: its damaged units are empty, and a context does not refuse a packet of no bytes
    (heaac_codec_decode returns 0 for it without calling the decoder)."""
    from test_shim_gpu import HeaacCodecContext, HeaacPacket
    lib = pkg.lib()
    T = 5
    m4, cfg, n, units, where, damaged = _damage(pkg, name, T)
    _both_refusal_kinds_occur(pkg, name, m4, damaged)
    got, status = _reference(pkg, m4, cfg, n, units, K * T)
    asc, length, nout = CODEC[name]
    assert got.shape == (K * T, n, length, nout)
    codec = C.c_void_p.in_dll(lib, "heaac_aac_decoder")
    out = (C.c_int16 * (192000 // 2))()
    for i in range(n):
        if i == 5:
            continue
        ctx = HeaacCodecContext(cfg=-1, extradata=asc, extradata_size=len(asc))
        assert lib.heaac_codec_open(C.byref(ctx), C.c_void_p(C.addressof(codec))) == 0
        refused = []
        for u in range(K * T):
            b = units[i][u]
            buf = C.create_string_buffer(b, len(b))
            pkt = HeaacPacket(C.cast(buf, C.c_void_p), len(b))
            size = C.c_int(192000)
            used = lib.heaac_codec_decode(C.byref(ctx), out, C.byref(size), C.byref(pkt))
            if used < 0:
                assert status[u][i] < 0 and not got[u][i].any(), (name, i, u, used, int(status[u][i]))
                refused.append(u)
                continue
            assert size.value == length * nout * 2, (name, i, u)
            pcm = np.frombuffer(out, np.int16, length * nout).reshape(length, nout)
            assert np.array_equal(pcm, got[u][i]), (name, i, u, int(status[u][i]))
        assert lib.heaac_codec_close(C.byref(ctx)) == 0
        # exactly the damaged units are refused, and the stream is heard again after them
        assert refused == sorted(where.get(i, [])), (name, i, refused)
        assert got[max(refused) + 1:, i].any() if refused else got[:, i].any(), (name, i)
