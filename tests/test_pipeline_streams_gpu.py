"""The pipeline's streams form (heaac_pipeline_create_streams: T access units per stream and tick, the streams calls with
hold masks on the GPU) against the pipeline as it was: Pipeline(..., frames_per_tick=1), fed the same units over K * T
ticks, runs the batch calls with the failed streams' state parked around them.  PCM and status bit for bit; later ticks
depend on the state carried across the tick boundary, so the state is covered through the PCM."""
import copy
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
