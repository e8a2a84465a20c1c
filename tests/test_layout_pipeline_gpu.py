"""include/heaac_pipeline.h, second half: heaac_layout_pipeline_* -- n streams of one multi-element layout through the
batched records (VERDICT r03 "missing" #2: aac_decode_frame's element loop, aacdec.c:1999-2076, had existed only behind
one heaac_codec_decode context per stream).  Every stream is ALSO decoded by a codec context of its own on the same
bytes (the path tests/test_layout_gpu.py pins to the oracle): the pipeline's interleaved int16 PCM must equal it
stream for stream and tick for tick -- 5.1 AAC-LC, 5.0 AAC-Main (predictor state per element and stream), 5.1 HE-AAC
with explicit SBR per element.  A damaged unit gives its stream silence on both paths, and both go on alike."""
import copy
import ctypes as C

import numpy as np
import pytest

import test_layout_gpu as LG

pytestmark = pytest.mark.gpu

SCE, CPE, CCE, LFE = 0, 1, 2, 3
UNSUPPORTED = -3                # HEAAC_PARSE_ERR_UNSUPPORTED: also the status of a unit the pipeline drops


def _decode(lib, ctx, b, out):
    from test_shim_gpu import HeaacPacket
    buf = C.create_string_buffer(b, len(b))
    pkt = HeaacPacket(C.cast(buf, C.c_void_p), len(b))
    size = C.c_int(192000)
    return lib.heaac_codec_decode(C.byref(ctx), out, C.byref(size), C.byref(pkt)), size.value


class _NeverGiven:
    """One heaac_codec_decode context per stream that is never given the units the pipeline drops: a unit that
    parses but deviates from the tick (element order, coupling places) must leave its stream as if it had never
    arrived.  feed(unit, status) returns (used, size), or None for a dropped unit.  A unit with status
    HEAAC_PARSE_ERR_UNSUPPORTED is tried on a fresh context that replays the stream first: where the codec refuses it
    too, the refusal is the parser's (and moves what the reference's decoder moves), and the fresh context takes
    over; where the codec decodes it, the pipeline dropped it."""
    def __init__(self, lib, asc):
        self.lib, self.asc, self.fed = lib, asc, []
        self.out = (C.c_int16 * (192000 // 2))()
        self.ctx = self._open()

    def _open(self):
        from test_shim_gpu import HeaacCodecContext
        codec = C.c_void_p.in_dll(self.lib, "heaac_aac_decoder")
        ctx = HeaacCodecContext(cfg=-1, extradata=self.asc, extradata_size=len(self.asc))
        assert self.lib.heaac_codec_open(C.byref(ctx), C.c_void_p(C.addressof(codec))) == 0
        return ctx

    def feed(self, b, status):
        if status == UNSUPPORTED:
            ctx = self._open()
            for u in self.fed:
                _decode(self.lib, ctx, u, self.out)
            used, size = _decode(self.lib, ctx, b, self.out)
            if used >= 0:
                assert self.lib.heaac_codec_close(C.byref(ctx)) == 0
                return None
            assert self.lib.heaac_codec_close(C.byref(self.ctx)) == 0
            self.ctx = ctx
        else:
            used, size = _decode(self.lib, self.ctx, b, self.out)
        self.fed.append(b)
        return used, size

    def pcm(self, length, nch):
        return np.frombuffer(self.out, np.int16, length * nch).reshape(length, nch)

    def close(self):
        assert self.lib.heaac_codec_close(C.byref(self.ctx)) == 0


def _stream_units(pkg, rng, mode, ticks):
    """The access units of one stream (raw data blocks), written as tests/test_layout_gpu.py writes them."""
    import sbr_bitwriter as SW
    import test_parse_layout as TL
    cc, elems, he, how = LG.MODES[mode]
    aot = 1 if mode.startswith("main") else 2
    si = 6 if he else 3
    ps_sce = he and cc == 0                     # program config element + explicit SBR: Parametric Stereo on every SCE
    writers = {k: SW.SbrStreamWriter(pkg, 2 if t == CPE else 1, ps=ps_sce and t == SCE) for k, (t, _) in enumerate(elems)}
    units = []
    for t in range(ticks):
        payloads = None
        if he:
            payloads = []
            for k, (typ, _) in enumerate(elems):
                if typ == LFE:
                    payloads.append(None)
                    continue
                w = writers[k]
                while True:
                    keep = copy.deepcopy((w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling))
                    bits, _ = w.frame(rng, new_header=(t == 3 and k == 1), respec=(t == 3 and k == 1))
                    if (4 + len(bits) + 7) // 8 <= 269:
                        break
                    w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling = keep
                payloads.append(bits)
        au, _ = TL.build(rng, si, aot, elems, extras=t & 1, payloads=payloads)
        units.append(au)
    return units, aot, si, cc, he


@pytest.mark.parametrize("mode", ["lc_5_1", "main_5_0", "he_5_1", "he_pce_ps_3_0", "he_pce_ps_5_1_downsampled"])
def test_layout_pipeline_equals_one_codec_context_per_stream(pkg, dev, mode):
    import test_parse as TP
    from test_shim_gpu import HeaacCodecContext, HeaacPacket
    lib = pkg.lib()
    n, ticks = 6, 5
    rng = np.random.default_rng(sum(map(ord, mode)) + 9)
    streams = [_stream_units(pkg, rng, mode, ticks) for _ in range(n)]
    _, aot, si, cc, he = streams[0]
    pce = None
    if cc == 0:
        import test_parse_layout as TL
        elems = LG.MODES[mode][1]
        front = [(int(t == CPE), g) for t, g in elems if t in (SCE, CPE) and not (t == CPE and g == 1)]
        pce = lambda bw: TL.write_pce_body(bw, np.random.default_rng(1), front, [], [(1, 1)] if (CPE, 1) in elems else [],
                                           [g for t, g in elems if t == LFE])
    down = LG.MODES[mode][3] == "asc_downsampled"
    asc = LG._asc(aot, si, cc, he=he, pce=pce, ext_si=si if down else None)
    r, m4, layout = pkg.asc_layout(asc)
    assert r == 0
    if not he:
        assert m4.sbr == -1          # a plain AAC-LC configuration leaves implicit SBR open; these streams carry none
        m4.sbr = 0
    # a single channel element with Parametric Stereo gives two channels (aacdec.c:203-206)
    nch = int(layout[0]["channels"]) + (sum(t == SCE for t, _ in LG.MODES[mode][1]) if he and cc == 0 else 0)
    length = 2048 if he and not down else 1024
    # one damaged unit: its stream gets silence for that tick
    bad_tick, bad = 2, 4
    units = [[streams[i][0][t] for i in range(n)] for t in range(ticks)]
    fed = [list(u) for u in units]
    fed[bad_tick][bad] = units[bad_tick][bad][:6] + bytes(8)

    # the reference run: a codec context per stream
    codec = C.c_void_p.in_dll(lib, "heaac_aac_decoder")
    want = np.zeros((ticks, n, length, nch), np.int16)
    out = (C.c_int16 * (192000 // 2))()
    for i in range(n):
        ctx = HeaacCodecContext(cfg=-1, extradata=asc, extradata_size=len(asc))
        assert lib.heaac_codec_open(C.byref(ctx), C.c_void_p(C.addressof(codec))) == 0
        for t in range(ticks):
            if t == bad_tick and i == bad:
                # refused: no samples (what the refused unit leaves behind in the stream -- window history, noise
                # generator, predictors as far as the reference's decoder had got, tests/test_refused_units.py -- is
                # the same on both paths)
                b = fed[t][i]
                buf = C.create_string_buffer(b, len(b))
                pkt = HeaacPacket(C.cast(buf, C.c_void_p), len(b))
                size = C.c_int(192000)
                assert lib.heaac_codec_decode(C.byref(ctx), out, C.byref(size), C.byref(pkt)) < 0
                continue
            b = units[t][i]
            buf = C.create_string_buffer(b, len(b))
            pkt = HeaacPacket(C.cast(buf, C.c_void_p), len(b))
            size = C.c_int(192000)
            assert lib.heaac_codec_decode(C.byref(ctx), out, C.byref(size), C.byref(pkt)) == len(b), (i, t)
            assert size.value == length * nch * 2
            want[t, i] = np.frombuffer(out, np.int16, size.value // 2).reshape(length, nch)
        assert lib.heaac_codec_close(C.byref(ctx)) == 0

    pl = pkg.LayoutPipeline(m4, layout, n, threads=3)
    assert pl.ch == nch
    got = []
    for t in range(ticks):
        st = pl.submit(fed[t])
        if t == bad_tick:
            assert st[bad] < 0 and all(st[i] == 0 for i in range(n) if i != bad)
        else:
            assert (st == 0).all(), (t, st)
        if t >= 1:
            got.append(pl.collect().copy())
    got.append(pl.collect().copy())
    with pytest.raises(pkg.HeaacError):
        pl.collect()
    for t in range(ticks):
        assert got[t].shape == (n, length, nch)
        for i in range(n):
            assert np.array_equal(got[t][i], want[t, i]), ("tick %d stream %d" % (t, i), np.argwhere(got[t][i] != want[t, i])[:3])
    assert not got[bad_tick][bad].any() and int(np.abs(got[ticks - 1][bad].astype(int)).max()) > 20
    pl.close()


def test_layout_pipeline_refuses_what_it_does_not_take(pkg, dev):
    import test_parse as TP
    r, layout = pkg.aac_layout_default(6)
    assert r == 0
    m4 = TP._cfg(pkg, 2, 3, 6)
    m4.sbr = -1                                                # implicit signalling: settled per stream
    with pytest.raises(pkg.HeaacError):
        pkg.LayoutPipeline(m4, layout, 4)
    m4.sbr = 0
    l2 = layout.copy()
    l2[0]["slot_of"][2][5] = 1                                 # a coupling channel element in the layout ...
    l2[0]["slot_of"][2][6] = 17                                # ... in a slot the layout's list cannot have
    with pytest.raises(pkg.HeaacError):
        pkg.LayoutPipeline(m4, l2, 4)
    pl = pkg.LayoutPipeline(m4, layout, 4)
    for _ in range(2):
        pl.submit([bytes(16)] * 4)                             # (garbage units: every stream fails, silence)
    with pytest.raises(pkg.HeaacError):
        pl.submit([bytes(16)] * 4)                             # a third tick in flight
    assert not pl.collect().any()
    pl.close()


@pytest.mark.parametrize("seed", list(range(int(__import__("os").environ.get("HEAAC_FUZZ_SEEDS", "1")))))
@pytest.mark.parametrize("mode", ["lc_5_1", "main_5_0", "he_5_1", "he_pce_ps_3_0"])
def test_layout_pipeline_and_codec_agree_on_damaged_streams(pkg, dev, mode, seed):
    """Mutated access units (bit flips, byte noise, truncation, splices) through the layout pipeline and through one
    codec context per stream: the same verdict unit for unit -- refused and silent, or the same PCM -- and the same
    streams afterwards (what a refused unit leaves behind is followed up per element on both paths,
    tests/test_refused_units.py)."""
    from test_damaged_streams_gpu import _mutate
    from test_shim_gpu import HeaacCodecContext, HeaacPacket
    lib = pkg.lib()
    n, ticks = 16, 9
    rng = np.random.default_rng(sum(map(ord, mode)) + 77 + 1000 * seed)
    streams = [_stream_units(pkg, rng, mode, ticks) for _ in range(n)]
    _, aot, si, cc, he = streams[0]
    pce = None
    if cc == 0:
        import test_parse_layout as TL
        elems = LG.MODES[mode][1]
        front = [(int(t == CPE), g) for t, g in elems if t in (SCE, CPE) and not (t == CPE and g == 1)]
        pce = lambda bw: TL.write_pce_body(bw, np.random.default_rng(1), front, [], [(1, 1)] if (CPE, 1) in elems else [],
                                           [g for t, g in elems if t == LFE])
    asc = LG._asc(aot, si, cc, he=he, pce=pce)
    r, m4, layout = pkg.asc_layout(asc)
    assert r == 0
    if not he:
        m4.sbr = 0
    units = [[streams[i][0][t] for i in range(n)] for t in range(ticks)]
    pool = [u for tick in units for u in tick]
    fed = [list(u) for u in units]
    for t in range(2, ticks):
        for i in range(n):
            if rng.random() < 0.4:
                fed[t][i] = _mutate(rng, fed[t][i], pool)
    # one unit with its first two elements swapped: the codec takes it (the tags are mapped by then), the pipeline
    # wants the order its first good unit set and drops it
    import test_parse_layout as TL
    elems = LG.MODES[mode][1]
    fed[3][5] = TL.build(np.random.default_rng(3), si, aot, [elems[1], elems[0]] + list(elems[2:]), extras=False)[0]
    pl = pkg.LayoutPipeline(m4, layout, n, threads=3)
    nch, length = pl.ch, pl.len
    got, status = [], []
    for t in range(ticks):
        status.append(np.array(pl.submit(fed[t])).copy())
        got.append(pl.collect().copy())
    pl.close()
    refused = after = dropped = 0
    for i in range(n):
        model = _NeverGiven(lib, asc)
        seen = False
        for t in range(ticks):
            r = model.feed(fed[t][i], int(status[t][i]))
            if r is None:
                # dropped (the pipeline wants one element order for all its streams): silence, and from here on the
                # stream is what a codec context is that never saw the unit
                assert not got[t][i].any(), (mode, i, t)
                dropped += 1
                seen = True
                continue
            used, size = r
            if used < 0:
                assert status[t][i] < 0 and not got[t][i].any(), (mode, i, t, int(status[t][i]))
                refused += 1
                seen = True
                continue
            assert status[t][i] == 0 and size == length * nch * 2, (mode, i, t, int(status[t][i]))
            assert np.array_equal(model.pcm(length, nch), got[t][i]), (mode, i, t)
            after += seen
        model.close()
    assert refused > n // 3 and after > n // 2 and dropped >= 1 and status[3][5] == UNSUPPORTED


def _coupled_unit(rng, si, aot, elems, tags, at, points, payloads=None, cce_payloads=None, quiet=False):
    """An access unit of a layout with coupling elements, as tests/coupled_ref.py writes them, but with the elements
    in the given order and coupling element `tags[k]` in front of output element number `at[k]` (len(elems): behind
    the last): the order every stream of a pipeline shares.  Targets, gain lists and coupling points are drawn."""
    import aac_bitwriter as W
    import coupled_ref as CR
    import test_parse_layout as TL
    import test_parse_wide as TW
    real = [e for e in elems if e[0] != LFE]
    bw = W.BitWriter()
    for pos in range(len(elems) + 1):
        for k, tag in enumerate(tags):
            if at[k] != pos:
                continue
            targets = []
            for _ in range(int(rng.integers(1, 3))):
                t, g = real[int(rng.integers(0, len(real)))]
                targets.append((t, g, int(rng.integers(0, 4)) if t == CPE else 2))
            TW.write_cce(bw, rng, si, aot, tag, targets, int(rng.choice(points)), quiet=quiet)
            if cce_payloads and cce_payloads.get(tag) is not None:
                CR.put_sbr_fill(bw, cce_payloads[tag])
        if pos < len(elems):
            TL.write_elem(bw, rng, si, aot, *elems[pos], quiet=quiet)
            if payloads and payloads.get(pos) is not None:
                CR.put_sbr_fill(bw, payloads[pos])
    bw.put(7, 3)
    return bw.bytes()


def _moved(at, n_elems):
    """Other places for the coupling elements (each one output element further on, cyclically)."""
    moved = sorted((a + 1) % (n_elems + 1) for a in at)
    assert moved != list(at)
    return moved


@pytest.mark.parametrize("name", ["five_one", "main_three", "pair_dependent", "mono_independent", "he_three_dependent", "he_three_all"])
def test_layout_pipeline_with_coupling_elements_equals_one_codec_context_per_stream(pkg, dev, name):
    """AAC-LC / Main layouts whose program config element names coupling channel elements (tests/test_coupling_gpu.py
    pins the codec path to the oracle on them): dependent coupling around every target's TNS, independent coupling
    behind its IMDCT -- the coupling point drawn per stream and unit, so that a tick mixes them -- onto one and onto
    several output elements; in the HE-AAC layouts the coupling channels go through SBR with payloads of their own and
    couple over 2048 samples.  Some units are damaged; one stream leaves a coupling element out for a unit."""
    import coupled_ref as CR
    import test_coupling_gpu as TC
    from test_damaged_streams_gpu import _mutate
    from test_shim_gpu import HeaacCodecContext, HeaacPacket
    lib = pkg.lib()
    aot, elems, cc_tags, points = TC.STREAMS[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 5)
    he = name.startswith("he_")
    si, n, ticks = (6 if he else 3), 10, 8
    length = 2048 if he else 1024
    asc = CR.asc(aot, si, elems, cc_tags, rng, he=he)
    r, m4, layout = pkg.asc_layout(asc)
    assert r == 0
    if not he:
        m4.sbr = 0
    nch = int(layout[0]["channels"])
    at = [int(x) for x in sorted(rng.integers(0, len(elems) + 1, len(cc_tags)))]
    # per stream: the SBR payload writers of its elements and coupling channels (HE layouts)
    uws = [CR.UnitWriter(pkg, rng, si, aot, elems, cc_tags, points, he) for _ in range(n)]

    def one(i, tags=None, places=None):
        uw = uws[i]
        tags = cc_tags if tags is None else tags
        pay = {k: uw._payload(w) for k, w in uw.writers.items()}
        cpay = {g: uw._payload(w) for g, w in uw.cce_writers.items() if g in tags}
        return _coupled_unit(rng, si, aot, elems, tags, at if places is None else places, points, pay, cpay, quiet=he)

    fed = [[one(i) for i in range(n)] for _ in range(ticks)]
    pool = [u for t in fed for u in t]
    for t in range(2, ticks):
        for i in range(n):
            if rng.random() < 0.25:
                fed[t][i] = _mutate(rng, fed[t][i], pool)
    fed[4][3] = one(3, cc_tags[:-1], at[:-1])              # a coupling element left out: refused
    fed[5][6] = one(6, places=_moved(at, len(elems)))      # the coupling elements elsewhere in the unit: dropped
    pl = pkg.LayoutPipeline(m4, layout, n, threads=3)
    assert pl.ch == nch and pl.len == length
    got, status = [], []
    for t in range(ticks):
        status.append(np.array(pl.submit(fed[t])).copy())
        got.append(pl.collect().copy())
    pl.close()
    decoded = refused = dropped = 0
    for i in range(n):
        model = _NeverGiven(lib, asc)
        for t in range(ticks):
            r = model.feed(fed[t][i], int(status[t][i]))
            if r is None:
                # (a unit that moved an element or a coupling element: the pipeline wants one order and one place of the
                # coupling elements for all streams of a tick) -- silence, and the stream goes on as if it never came
                assert not got[t][i].any(), (name, i, t)
                dropped += 1
                continue
            used, size = r
            if used < 0:
                assert status[t][i] < 0 and not got[t][i].any(), (name, i, t, int(status[t][i]))
                refused += 1
                continue
            # (a negative status with samples: an SBR payload that failed behind a damaged unit -- SBR off for the unit)
            assert size == length * nch * 2, (name, i, t, int(status[t][i]))
            pcm = model.pcm(length, nch)
            assert np.array_equal(pcm, got[t][i]), (name, i, t, np.argwhere(pcm != got[t][i])[:3])
            decoded += 1
        model.close()
    assert status[4][3] < 0 and decoded > n * ticks // 2 and refused >= 1 and dropped >= 1
    assert max(int(np.abs(g.astype(int)).max()) for g in got) > 50


def _coupled_streams(pkg, name, seed, n_distinct):
    """The setup of the coupling tests: (asc, m4, layout, nch, length, unit(i, order=None, places=None))."""
    import coupled_ref as CR
    import test_coupling_gpu as TC
    aot, elems, cc_tags, points = TC.STREAMS[name]
    rng = np.random.default_rng(seed)
    he = name.startswith("he_")
    si = 6 if he else 3
    asc = CR.asc(aot, si, elems, cc_tags, rng, he=he)
    r, m4, layout = pkg.asc_layout(asc)
    assert r == 0
    if not he:
        m4.sbr = 0
    at = [int(x) for x in sorted(rng.integers(0, len(elems) + 1, len(cc_tags)))]
    uws = [CR.UnitWriter(pkg, rng, si, aot, elems, cc_tags, points, he) for _ in range(n_distinct)]

    def unit(i, order=None, places=None):
        """Stream i's next unit; `order`: its output elements in this order (a permutation of the layout's list)."""
        uw = uws[i]
        order = list(range(len(elems))) if order is None else order
        pay = {k: uw._payload(w) for k, w in uw.writers.items()}
        cpay = {g: uw._payload(w) for g, w in uw.cce_writers.items()}
        return _coupled_unit(rng, si, aot, [elems[k] for k in order], cc_tags, at if places is None else places, points,
                             {pos: pay.get(k) for pos, k in enumerate(order)}, cpay, quiet=he)

    def writers(i):
        return list(uws[i].writers.values()) + list(uws[i].cce_writers.values())

    unit.writers, unit.at, unit.n_elems = writers, at, len(elems)
    return asc, m4, layout, int(layout[0]["channels"]), 2048 if he else 1024, unit


@pytest.mark.parametrize("name", ["five_one", "he_three_all"])
@pytest.mark.parametrize("how", ["swapped_elements", "moved_coupling_element"])
def test_a_dropped_unit_leaves_its_stream_as_if_it_had_never_come(pkg, dev, name, how):
    """a unit that parses but deviates from the tick -- two output elements swapped, or the coupling
    elements at other places than the tick's -- is dropped after the parse (status HEAAC_PARSE_ERR_UNSUPPORTED,
    silence).  Its stream's host state (window histories, SBR readers, header table entries, coupling elements seen)
    must stay with its parked device rows: every later tick of that stream is bit for bit a codec context's that was
    never given the unit, and the other streams of the tick are untouched.  AAC-LC 5.1 with two coupling elements;
    HE-AAC 3.0 + LFE whose coupling channels also couple behind the IMDCT, through SBR of their own."""
    import copy
    lib = pkg.lib()
    n, ticks, drop_tick, j = 6, 6, 2, 3
    asc, m4, layout, nch, length, unit = _coupled_streams(pkg, name, sum(map(ord, name + how)), n)
    fed = []
    for t in range(ticks):
        row = []
        for i in range(n):
            if (t, i) != (drop_tick, j):
                row.append(unit(i))
                continue
            # (the payload writers of the stream are put back behind the dropped unit: the next unit's SBR payloads
            # follow the last one the decoder has seen)
            keep = [copy.deepcopy((w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling)) for w in unit.writers(i)]
            if how == "swapped_elements":
                order = list(range(unit.n_elems))
                order[0], order[1] = 1, 0
                row.append(unit(i, order=order))
            else:
                row.append(unit(i, places=_moved(unit.at, unit.n_elems)))
            for w, k in zip(unit.writers(i), keep):
                w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling = k
        fed.append(row)
    pl = pkg.LayoutPipeline(m4, layout, n, threads=3)
    assert pl.ch == nch and pl.len == length
    got, status = [], []
    for t in range(ticks):
        status.append(np.array(pl.submit(fed[t])).copy())
        got.append(pl.collect().copy())
    pl.close()
    for t in range(ticks):
        for i in range(n):
            assert status[t][i] == (UNSUPPORTED if (t, i) == (drop_tick, j) else 0), (t, i, int(status[t][i]))
    assert not got[drop_tick][j].any()
    for i in range(n):
        model = _NeverGiven(lib, asc)
        for t in range(ticks):
            r = model.feed(fed[t][i], int(status[t][i]))
            if (t, i) == (drop_tick, j):
                assert r is None                    # the codec decodes the unit: only the pipeline drops it
                continue
            used, size = r
            assert used == len(fed[t][i]) and size == length * nch * 2, (t, i, used)
            pcm = model.pcm(length, nch)
            assert np.array_equal(pcm, got[t][i]), (how, t, i, np.argwhere(pcm != got[t][i])[:3])
        model.close()
    assert all(got[t][j].any() for t in range(drop_tick + 1, ticks))


def test_a_tick_of_thousands_of_units_per_slice_with_spectrum_coupling_and_no_payload(pkg, dev):
    """8 192 HE-AAC streams of a 3.0 + LFE layout on two parser threads (4 096 per slice), every unit with coupling
    elements that couple in the spectrum and carry no SBR payload of their own -- the case that took a copy of the
    coupling channel's SBR reader state on the stack for every stream of the slice, every tick.  The streams are
    copies of 16 distinct ones, each compared with one heaac_codec_decode context per distinct stream."""
    distinct, n, ticks = 16, 8192, 3
    lib = pkg.lib()
    asc, m4, layout, nch, length, unit = _coupled_streams(pkg, "he_three_dependent", 4096, distinct)
    units = [[unit(j) for j in range(distinct)] for _ in range(ticks)]
    pl = pkg.LayoutPipeline(m4, layout, n, threads=2)
    got = []
    for t in range(ticks):
        st = np.array(pl.submit([units[t][i % distinct] for i in range(n)])).copy()
        assert (st == 0).all(), t
        got.append(pl.collect().copy())
    pl.close()
    for j in range(distinct):
        model = _NeverGiven(lib, asc)
        for t in range(ticks):
            used, size = model.feed(units[t][j], 0)
            assert used == len(units[t][j]) and size == length * nch * 2, (j, t, used)
            copies = got[t][j::distinct]
            assert copies.shape[0] == n // distinct and (copies == model.pcm(length, nch)[None]).all(), (j, t)
        model.close()
    assert max(int(np.abs(g.astype(int)).max()) for g in got) > 50
