"""The device-parse pipeline (heaac_pipeline_create_ex with HEAAC_PIPELINE_DEVICE_PARSE: units packed and uploaded as
they are, parsed by the streams walk on the GPU, the streams it stops finished by the host parser and scattered into the
tick's rows) against the host-parse pipeline fed the same units: PCM and status bit for bit, for clean, deferred,
damaged, empty and SBR-only-damaged units.  parse_counts() is held against a model made on the CPU from the walk's host
form, so that a build which hands everything to the host parser does not pass.

The corpora and helpers are those of tests/test_pipeline_streams_gpu.py (K = 3 ticks, all submitted before the first
collect; n = 7 streams); the reference is its one-unit host-parse pipeline."""
import copy

import numpy as np
import pytest

import parse_device_common as PC
import sbr_bitwriter as SW
import sbr_device_common as SD
import test_parse as TP
import test_pipeline_streams_gpu as PS
import test_sbr_parse as TS

pytestmark = pytest.mark.gpu

K = PS.K
TS_PER_TICK = [1, 2, 5]
CASES = PS.CASES                 # hev2, hev1, hev1_down, lc_stereo_main, lc_mono

_refs = {}


def _clean_reference(pkg, name):
    """The one-unit host-parse pipeline over the case's first K * max(T) units, run once per case: every T reads a prefix"""
    if name not in _refs:
        m4, cfg, n, units, *_ = PS._case(pkg, name)
        ref, ref_status = PS._reference(pkg, m4, cfg, n, units, K * max(TS_PER_TICK))
        ref.setflags(write=False)
        ref_status.setflags(write=False)
        _refs[name] = (ref, ref_status)
    return _refs[name]


def _device(pkg, m4, cfg, n, units, T, threads, ticks=K):
    """`ticks` ticks of T units per stream through a device-parse pipeline, all submitted before the first collect:
    PCM [ticks][n][T][len][ch], status [ticks][n][T], parse_counts() after each submit"""
    pl = pkg.Pipeline(m4, cfg, n, threads=threads, frames_per_tick=T, device_parse=True)
    assert pl.parse_counts() == (0, 0)
    status, counts = [], []
    for k in range(ticks):
        status.append(np.array(pl.submit([units[i][k * T + t] for i in range(n) for t in range(T)])).copy().reshape(n, T))
        counts.append(pl.parse_counts())
    pcm = [pl.collect().copy().reshape((n, T) + (pl.len, pl.ch)) for _ in range(ticks)]
    with pytest.raises(pkg.HeaacError):
        pl.collect()                                  # nothing in flight
    tm = pl.timing()
    assert tm["parse"] > 0 and tm["gpu"] > 0
    assert pl.parse_counts() == counts[-1]
    pl.close()
    return np.stack(pcm), np.stack(status), counts


def _model_counts(pkg, name, m4, n, units, T, cc, ticks=K):
    """What parse_counts() must say after each tick, from the host forms alone.  Per tick the walk's host form
    (parse_core_streams: the chain the kernel instantiates) runs from the streams' states and says where each stream
    stops (t0); the states are then carried over the tick's T units by the host parser, as an all-host chain carries them
    -- which by the parsers' contract is byte for byte what the walk plus the resumed host parser leave.
    device += t0, host += T - t0."""
    he, with_ps = name.startswith("hev"), name == "hev2"
    st = np.zeros(n, pkg.AAC_STREAM_DT)
    sst = pkg.sbr_streams(n) if he else None
    tab = pkg.SbrHeaderTable(256) if he else None
    device = host = 0
    out = []
    for k in range(ticks):
        aus = [units[s][k * T + t] for s in range(n) for t in range(T)]
        if he:
            r = pkg.parse_core_streams(m4, st.copy(), aus, T, cc, sst_in=sst, hdr=tab.headers(), with_ps=with_ps)
        else:
            r = pkg.parse_core_streams(m4, st.copy(), aus, T, cc)
        t0 = int(np.asarray(r["taken"]).astype(np.int64).sum())
        device += t0
        host += n * T - t0
        out.append((device, host))
        for t in range(T):
            row = [units[s][k * T + t] for s in range(n)]
            if he:
                SD.host_parse(pkg, m4, st, sst, tab, row, cc, with_ps)
            else:
                PC.host_parse(pkg, m4, st, row, cc)
    if tab is not None:
        tab.close()
    return out


_shares = {}


def _device_share_at_one_unit_per_tick(pkg, name):
    """The condition under which equal PCM says something about the device: walked at T = 1 -- where a deferred unit
    costs the walk nothing but itself -- the device takes more than half of ALL the units of the case's corpus (the
    K * T_MAX = 24 units per stream the case draws).  Over the first K = 3 units alone an HE corpus cannot get there:
    each stream's first header is one of its three units and about four in ten units carry pulse data (hev2: 8 of 21,
    hev1_down: 9 of 21), so the share is taken over the corpus, of which every T walks a prefix."""
    if name not in _shares:
        m4, cfg, n, units, si, aot, channels = PS._case(pkg, name)
        _shares[name] = _model_counts(pkg, name, m4, n, units, 1, channels, ticks=len(units[0]))[-1]
    device, host = _shares[name]
    assert device + host == 7 * K * PS.T_MAX and device > (device + host) // 2, (name, device, host)


@pytest.mark.parametrize("T", TS_PER_TICK)
@pytest.mark.parametrize("name", CASES)
def test_device_parse_ticks_equal_host_parse_ticks(pkg, dev, name, T):
    """The LC corpora carry pulse-data units (good units the walk defers), the HE corpora each stream's first header and
    a new header at unit 3 (deferred as well): walk, fix-up and the walk resumed behind it, all in K ticks."""
    m4, cfg, n, units, si, aot, channels = PS._case(pkg, name)
    # on the CPU first: the device must do most of the parsing
    _device_share_at_one_unit_per_tick(pkg, name)
    want = _model_counts(pkg, name, m4, n, units, T, channels)
    assert want[-1][0] > 0 and want[-1][1] > 0, want  # walk and fix-up both have something to do in these K ticks
    ref, ref_status = _clean_reference(pkg, name)
    assert (ref_status[:K * T] >= 0).all()
    assert int(np.abs(ref[:K * T].astype(int)).max()) > 50
    got, status, counts = _device(pkg, m4, cfg, n, units, T, threads=2)
    PS._compare(got, status, ref[:K * T], ref_status[:K * T], n, T)
    assert counts == want, (counts, want)


def _sbr_only_failure(pkg, name, m4, units, u, si, aot):
    """units[6][u] replaced by a unit whose AAC element is good and whose SBR payload fails (a malformed grid of
    tests/test_sbr_parse.py: no header, no extra data, FIXFIX with 8 envelopes).  Checked on the CPU: the host parser
    answers a negative status WITH the channels read -- not a core failure: the unit decodes with SBR off."""
    rng = np.random.default_rng(303 + u)
    bits = [0, 0]
    for v, nb in TS.BAD_GRIDS[0]:
        bits += [(v >> (nb - 1 - k)) & 1 for k in range(nb)]
    bits += [0] * (64 - len(bits))
    units[6][u] = TP._write_au(rng, si, aot, False, extras=False, sbr=(bits, False), quiet=True)[0]
    st, sst, tab = np.zeros(1, pkg.AAC_STREAM_DT), pkg.sbr_streams(1), pkg.SbrHeaderTable(64)
    for v in range(u + 1):
        h = SD.host_parse(pkg, m4, st, sst, tab, [units[6][v]], 1, True)
    tab.close()
    assert h["status"][0] < 0 and h["info"]["channels"][0] == 1, (h["status"], h["info"])


@pytest.mark.parametrize("T", TS_PER_TICK)
@pytest.mark.parametrize("name", CASES)
def test_damaged_units_in_device_parse_ticks(pkg, dev, name, T):
    """The damaged units of tests/test_pipeline_streams_gpu.py -- refusals with and without HEAAC_REFUSED_RUN_TOOLS, the
    unit only this parser refuses, a whole tick of one stream, a stream run out of units -- and, for the mono HE case, a
    unit whose SBR payload alone fails (the CPE cases get none: neither tests/test_pipeline.py nor
    tests/test_sbr_parse.py writes a failing CPE payload)."""
    m4, cfg, n, units, where, damaged = PS._damage(pkg, name, T)
    PS._both_refusal_kinds_occur(pkg, name, m4, damaged)
    _, _, _, _, si, aot, channels = PS._case(pkg, name)
    sbr_only = K * T - 2 if name == "hev2" else None
    if sbr_only is not None:
        _sbr_only_failure(pkg, name, m4, units, sbr_only, si, aot)
    ref, ref_status = PS._reference(pkg, m4, cfg, n, units, K * T)
    for s, us in where.items():
        for u in us:
            assert ref_status[u][s] < 0 and not ref[u][s].any(), (s, u)
        # silence against silence would show nothing: the stream is heard again after its damaged units
        assert not us or ref[max(us) + 1:, s].any(), s
    if sbr_only is not None:
        assert ref_status[sbr_only][6] < 0 and ref[sbr_only][6].any()          # refused payload, decoded unit
    want = _model_counts(pkg, name, m4, n, units, T, channels)
    results = []
    for threads in (1, 2):
        got, status, counts = _device(pkg, m4, cfg, n, units, T, threads)
        PS._compare(got, status, ref, ref_status, n, T)
        assert counts == want, (threads, counts, want)
        results.append(got)
    assert np.array_equal(results[0], results[1])


@pytest.mark.parametrize("name", ["lc_stereo_main", "lc_mono"])
def test_a_corpus_without_pulse_data_never_reaches_the_host_parser(pkg, dev, name):
    """AAC-LC / Main units without pulse data (parse_device_common.no_pulses) are all in the walk's scope: the host count
    stays 0 over every tick, the PCM is the host-parse pipeline's, and the host-parse pipeline counts the other way."""
    m4, cfg, n, _, si, aot, channels = PS._case(pkg, name)
    T = 2
    rng = np.random.default_rng(41 + channels)
    with PC.no_pulses():
        units = [[TP._write_au(rng, si, aot, channels == 2, extras=True, quiet=True)[0] for _ in range(K * T)] for _ in range(n)]
    want = _model_counts(pkg, name, m4, n, units, T, channels)
    assert want == [(n * T * (k + 1), 0) for k in range(K)], want            # on the CPU, before the GPU run
    ref, ref_status = PS._reference(pkg, m4, cfg, n, units, K * T)
    assert (ref_status == 0).all() and int(np.abs(ref.astype(int)).max()) > 50
    got, status, counts = _device(pkg, m4, cfg, n, units, T, threads=2)
    PS._compare(got, status, ref, ref_status, n, T)
    assert counts == want, counts
    # without the flag: {0, units submitted}
    pl = pkg.Pipeline(m4, cfg, n, threads=2, frames_per_tick=T)
    pl.submit([units[i][t] for i in range(n) for t in range(T)])
    assert pl.parse_counts() == (0, n * T)
    pl.collect()
    pl.close()


def _reach_corpus(pkg, n, T, stops):
    """HE-AACv2 units[n][K * T] without pulse data and with no header but each stream's first -- so that after tick 0
    the walk takes everything -- except that stream s of `stops` carries pulse data in unit T + stops[s].  13 distinct
    streams are drawn and dealt out in turn (s mod 13): neighbouring rows differ, and the corpus is drawn in a second."""
    rng = np.random.default_rng(1300)
    base = 13
    writers = [SW.SbrStreamWriter(pkg, 1, ps=True, ps_modes="20") for _ in range(base)]
    drawn = [[] for _ in range(base)]
    special = {}
    for u in range(K * T):
        for b, w in enumerate(writers):
            while True:                               # (as tests/test_pipeline.py: a payload that fits its fill element)
                keep = copy.deepcopy((w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling))
                bits, _ = w.frame(rng, new_header=False)
                if (4 + len(bits) + 7) // 8 <= 269:
                    break
                w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling = keep
            with PC.no_pulses():
                drawn[b].append(TP._write_au(rng, 6, 2, False, extras=False, sbr=(bits, False), quiet=True)[0])
            for s, t0 in stops.items():
                if s % base == b and u == T + t0:     # the same payload behind an element with pulse data
                    while True:
                        au, e = TP._write_au(rng, 6, 2, False, extras=False, sbr=(bits, False), quiet=True)
                        if any(d["pulse"] for d in e["ch"]):
                            break
                    special[s] = au
    units = [list(drawn[s % base]) for s in range(n)]
    for s, t0 in stops.items():
        units[s][T + t0] = special[s]
    return units


def test_fix_up_reaches_every_wave_and_hands_the_streams_back_to_the_walk(pkg, dev):
    """n = 130 streams (three waves of 64 lanes, the last partial), T = 3.  Tick 0: every stream's first header, so the
    whole tick is staged and scattered row for row (rows of 7 132, 680 and 532 bytes: every alignment of the 16-byte
    copy).  Tick 1: streams 0, 63, 64 and 129 -- the first and last lanes of the waves -- stop at t0 = 0, 1, 2, 0 and no
    other stream does, so the staged rows of each land between rows of the device's own.  Tick 2: the device takes every
    unit again, the four streams' from the states the host parser left."""
    n, T = 130, 3
    stops = {0: 0, 63: 1, 64: 2, 129: 0}
    m4 = TS._he_cfg(pkg, 1, True)
    cfg = pkg.CFG_HEV2
    units = _reach_corpus(pkg, n, T, stops)
    rest = sum(T - t0 for t0 in stops.values())
    want = [(0, n * T), (n * T - rest, n * T + rest), (2 * n * T - rest, n * T + rest)]
    assert _model_counts(pkg, "hev2", m4, n, units, T, 1) == want            # on the CPU, before the GPU run
    ref, ref_status = PS._reference(pkg, m4, cfg, n, units, K * T)
    assert (ref_status >= 0).all() and int(np.abs(ref.astype(int)).max()) > 50
    got, status, counts = _device(pkg, m4, cfg, n, units, T, threads=2)
    PS._compare(got, status, ref, ref_status, n, T)
    assert counts == want, (counts, want)
