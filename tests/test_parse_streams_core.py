"""The chains of heaac_aac_parse_device_streams / heaac_heaac_parse_device_streams on the host (csrc/parse_streams.h
through heaac_debug_aac_parse_core_streams / heaac_debug_heaac_parse_core_streams): T consecutive units per stream in
one call, against the model of parse_streams_common.py -- the one-unit forms position by position, stopped streams
masked out, states put back -- and against the host parser: what is taken comes back byte for byte, a stream stops at
the first unit either one-unit form would defer, and from the states the call leaves the host parser resumes at that
unit with nothing to parse again."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import parse_device_common as PC
import parse_streams_common as PS
import sbr_device_common as SD
import test_parse as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg-heaac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")
CASES = [(False, 2, 3), (True, 2, 3), (True, 1, 4), (False, 2, 6), (True, 2, 11), (False, 1, 4)]      # test_parse_core.py's


def call_aac(pkg, cfg, st, rows, cc):
    """One streams call on `st` (updated in place), every output FILLed ahead of it."""
    T, S = len(rows), len(rows[0])
    return pkg.parse_core_streams(cfg, st, PS.flat(rows), T, coeff_channels=cc, out=PS.filled_streams(pkg, S, T, cc))


def call_he(pkg, cfg, st, sst, hdr, rows, cc, with_ps):
    T, S = len(rows), len(rows[0])
    return pkg.parse_core_streams(cfg, st, PS.flat(rows), T, coeff_channels=cc, sst_in=sst, hdr=hdr, with_ps=with_ps,
                                  out=PS.filled_streams(pkg, S, T, cc, sst, with_ps))


def run_aac(pkg, cfg, st, rows, cc, host_check=True):
    """The call against the model and the host parser; st moves on.  Returns (got, model)."""
    T, S = len(rows), len(rows[0])
    st0 = st.copy()
    mdl = PS.model(pkg, PS.HostOne(pkg), cfg, st0, rows, cc, host_check=host_check)
    got = call_aac(pkg, cfg, st, rows, cc)
    PS.compare_with_model(pkg, got, st, mdl, S, T)
    PS.check_against_host(pkg, cfg, got, st, st0, rows, cc)
    why = got["why"].reshape(S, T)
    for s in range(S):
        t0 = int(got["taken"][s])
        assert not why[s, :t0].any() and (why[s, t0 + 1:] == pkg.PARSE_WHY_STOPPED).all()
        assert t0 == T or 0 < why[s, t0] < pkg.PARSE_WHY_STOPPED
    return got, mdl


class HeChain:
    """S writer streams of one kind behind their first header (parsed on the host: the device never registers one)."""

    def __init__(self, pkg, rng, S, cpe, ps_modes="any"):
        self.pkg, self.S, self.cpe = pkg, S, cpe
        self.cfg = SD.he_cfg(pkg, cpe)
        self.with_ps, self.cc = not cpe, 2 if cpe else 1
        self.tab = pkg.SbrHeaderTable(64)
        self.st = np.zeros(S, pkg.AAC_STREAM_DT)
        self.sst = pkg.sbr_streams(S)
        self.writers = SD.make_writers(pkg, S, cpe, ps_modes)
        for _ in range(2):
            host = SD.host_parse(pkg, self.cfg, self.st, self.sst, self.tab, SD.he_units(rng, self.writers, cpe), self.cc, self.with_ps)
            assert not host["status"].any()

    def run(self, rows, host_check=True):
        pkg, S, T = self.pkg, self.S, len(rows)
        st0, sst0, hdr = self.st.copy(), self.sst.copy(), self.tab.headers()
        mdl = PS.model(pkg, PS.HostOne(pkg), self.cfg, st0, rows, self.cc, sst0, hdr, self.with_ps, self.tab, host_check)
        got = call_he(pkg, self.cfg, self.st, sst0, hdr, rows, self.cc, self.with_ps)
        PS.compare_with_model(pkg, got, self.st, mdl, S, T)
        PS.check_against_host(pkg, self.cfg, got, self.st, st0, rows, self.cc, sst0, self.tab, self.with_ps)
        self.sst = got["sst"]
        return got, mdl


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("cpe,aot,si", CASES)
def test_in_scope_aac_chains_are_taken_whole(pkg, cpe, aot, si, T):
    rng = np.random.default_rng(9100 + 7 * si + cpe + 100 * aot)
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    n, steps = 40, 4
    for adts in (0.0, 1.0):
        rows = PC.in_scope_steps(rng, si, aot, cpe, n, steps, adts=adts, sbr=0.3)
        for cc in ((2,) if cpe else (1, 2)):
            st = np.zeros(n, pkg.AAC_STREAM_DT)
            for k in range(0, steps, T):
                got, _ = run_aac(pkg, cfg, st, rows[k:k + T], cc)
                assert (got["taken"] == T).all(), ("the deferred share must be exactly 0", got["taken"], got["why"])
                assert not got["status"].any() and not got["hold"].any()
            assert st["oc"].all() and st["mapped_tag"].all()


@pytest.mark.parametrize("T", [1, 2, 4])
@pytest.mark.parametrize("cpe,ps_modes", SD.STREAMS)
def test_in_scope_he_chains_are_taken_whole(pkg, cpe, ps_modes, T):
    rng = np.random.default_rng(9200 + 10 * cpe + T + (0 if ps_modes in (None, "any") else int(ps_modes)))
    S = 12
    ch = HeChain(pkg, rng, S, cpe, ps_modes)
    rows = [SD.he_units(rng, ch.writers, cpe, crc=bool(t & 1)) for t in range(4)]
    for k in range(0, 4, T):
        got, _ = ch.run(rows[k:k + T])
        assert (got["taken"] == T).all(), ("the deferred share must be exactly 0", got["taken"], got["why"])
        assert not got["status"].any() and not got["hold"].any()
        assert (got["sbr"]["start"] == 1).all()


AAC_STOPS, HE_STOPS, aac_stop_unit = PS.AAC_STOPS, PS.HE_STOPS, PS.aac_stop_unit


@pytest.mark.parametrize("cpe,aot,si", [(False, 2, 3), (True, 2, 3), (True, 1, 4)])
def test_an_aac_stream_stops_at_its_first_deferred_unit(pkg, cpe, aot, si):
    rng = np.random.default_rng(9300 + cpe + aot)
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    T = 4
    plan = PS.stop_plan(rng, AAC_STOPS, [0, 1, T - 1], T)
    S = len(plan)
    rows = PC.in_scope_steps(rng, si, aot, cpe, S, T, adts=0.3, sbr=0.3)
    for s, (kind, t0) in enumerate(plan):
        if kind:
            rows[t0][s] = aac_stop_unit(rng, si, aot, cpe, kind, rows[t0][s])
    st = np.zeros(S, pkg.AAC_STREAM_DT)
    got, mdl = run_aac(pkg, cfg, st, rows, 2)
    assert [int(x) for x in got["taken"]] == [t0 for _, t0 in plan]
    why = got["why"].reshape(S, T)
    want = dict(pulse=pkg.PARSE_WHY_PULSE, cce=pkg.PARSE_WHY_ELEMENT, second_sce=pkg.PARSE_WHY_ELEMENT)
    for s, (kind, t0) in enumerate(plan):
        if kind:
            assert why[s, t0] == want.get(kind, pkg.PARSE_WHY_REFUSED), (s, kind, why[s])
            assert got["hold"].reshape(S, T)[s].tolist() == [0] * t0 + [1] * (T - t0)


@pytest.mark.parametrize("cpe", [False, True])
def test_an_he_stream_stops_at_the_first_unit_either_half_gives_up(pkg, cpe):
    rng = np.random.default_rng(9400 + cpe)
    T = 4
    plan = [(k or "plain", t0) for k, t0 in PS.stop_plan(rng, HE_STOPS, [0, 1, T - 1], T, whole=2)]
    S = len(plan)
    ch = HeChain(pkg, rng, S, cpe)
    rows = [SD.mixed_units(rng, ch.writers, cpe, [kind if t == t0 else "plain" for kind, t0 in plan]) for t in range(T)]
    st0 = ch.st.copy()
    got, mdl = ch.run(rows)
    why = got["why"].reshape(S, T)
    sbr_alone = 0
    for s, (kind, t0) in enumerate(plan):
        if kind == "flipped":                                     # damage may pass for data: only the rules hold
            assert int(got["taken"][s]) >= t0
            continue
        assert int(got["taken"][s]) == t0, (s, kind, got["taken"][s], why[s])
        if t0 < T:
            assert got["status"].reshape(S, T)[s].tolist() == [0] * t0 + [1] * (T - t0)
            assert got["hold"].reshape(S, T)[s].tolist() == [0] * t0 + [1] * (T - t0)
            if kind == "aac_refused":
                assert why[s, t0] == pkg.PARSE_WHY_REFUSED
            else:
                assert why[s, t0] >= pkg.PARSE_WHY_SBR and why[s, t0] % pkg.PARSE_WHY_SBR == 0
                sbr_alone += 1
    # where the SBR half alone gave the unit up the AAC half had taken it: its state was put back (compare_with_model
    # holds d_st against the model's, check_against_host lets the host parser resume from it)
    assert mdl["putback"] >= sbr_alone >= 12
    # a stream that stopped at its first unit is exactly as it was, in both halves
    first = np.array([t0 == 0 and kind != "flipped" for kind, t0 in plan])
    assert first.sum() >= 4
    assert np.array_equal(PC.rows(ch.st, S)[first], PC.rows(st0, S)[first])


def test_window_history_carries_inside_one_call(pkg):
    rng = np.random.default_rng(9500)
    cfg = TP._cfg(pkg, 2, 3, 2)
    S, T = 24, 4
    rows = PC.in_scope_steps(rng, 3, 2, True, S, T)
    st = np.zeros(S, pkg.AAC_STREAM_DT)
    got, _ = run_aac(pkg, cfg, st, rows, 2)
    assert (got["taken"] == T).all()
    ics = got["ics"].reshape(S, T, 2)
    for t in range(1, T):
        # (the second channel of a common-window pair takes the first one's sequences, and keeps its own shape)
        assert np.array_equal(ics["window_sequence"][:, t, 0, 1], ics["window_sequence"][:, t - 1, 0, 0])
        assert np.array_equal(ics["use_kb_window"][:, t, :, 1], ics["use_kb_window"][:, t - 1, :, 0])
    assert ics["window_sequence"][:, 1:, 0, 1].any() and ics["use_kb_window"][:, 1:, :, 1].any()
    assert np.array_equal(st["window_sequence"], ics["window_sequence"][:, T - 1, :, 0])


def test_implicit_ps_and_the_adts_lock_carry_inside_one_call(pkg):
    """test_parse_core.py::test_implicit_ps_and_tag_state_follow_the_host_parser as one T = 3 call."""
    rng = np.random.default_rng(31)
    cfg = TP._cfg(pkg, 2, 6, 1)
    cfg.sbr, cfg.ps = -1, -1
    S = 24
    rows = PC.in_scope_steps(rng, 6, 2, False, S, 3, adts=0.5, sbr=0.7)
    st = np.zeros(S, pkg.AAC_STREAM_DT)
    got, _ = run_aac(pkg, cfg, st, rows, 1)
    assert (got["taken"] == 3).all(), (got["taken"], got["why"])
    assert len(set(st["oc"].tolist())) > 1                       # locked with and without the implicit-PS re-configure


@pytest.mark.parametrize("cpe", [False, True])
def test_repeated_headers_and_units_without_payload_in_mid_chain_are_taken(pkg, cpe):
    rng = np.random.default_rng(9600 + cpe)
    S, T = 12, 3
    ch = HeChain(pkg, rng, S, cpe)
    mid = ["same_header" if s % 2 else "no_payload" for s in range(S)]
    rows = [SD.mixed_units(rng, ch.writers, cpe, mid if t == 1 else ["plain"] * S) for t in range(T)]
    got, _ = ch.run(rows)
    assert (got["taken"] == T).all(), (got["taken"], got["why"])
    start = got["sbr"]["start"].reshape(S, T)
    assert (start[0::2, 1] == 0).all() and (start[1::2, 1] == 1).all() and (start[:, 2] == 1).all()


def test_arguments(pkg):
    rng = np.random.default_rng(9700)
    S, T = 3, 2
    ch = HeChain(pkg, rng, S, False)
    rows = [SD.he_units(rng, ch.writers, False) for _ in range(T)]
    buf, off = pkg.pack_units(PS.flat(rows))
    off = off.astype(np.uint32)
    hdr = np.ascontiguousarray(ch.tab.headers())
    L = pkg.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)

    def outs():
        o = PS.filled_streams(pkg, S, T, 1, ch.sst, True)
        o["st"] = ch.st.copy()
        o["st"].view(np.uint8)[...] = PC.FILL
        return o

    def he(o, cfg=ch.cfg, S=S, T=T, cc=1, n_hdr=len(hdr), **null):
        a = dict(st=p(o["st"]), sst_in=p(ch.sst), sst=p(o["sst"]), au=p(buf), off=p(off), coeffs=p(o["coeffs"]),
                 ics=p(o["ics"]), tools=p(o["tools"]), info=p(o["info"]), hdr=p(hdr), sbr=p(o["sbr"]), ps=p(o["ps"]), status=p(o["status"]),
                 taken=p(o["taken"]), hold=p(o["hold"]))
        a.update(null)
        return L.heaac_debug_heaac_parse_core_streams(C.byref(cfg), a["st"], a["sst_in"], a["sst"], a["au"], a["off"], C.c_size_t(S),
                                                      C.c_size_t(T), cc, a["coeffs"], a["ics"], a["tools"], a["info"], a["hdr"],
                                                      C.c_size_t(n_hdr), a["sbr"], a["ps"], a["status"], a["taken"], a["hold"], None)

    def aac(o, cfg=ch.cfg, S=S, T=T, cc=1, **null):
        a = dict(st=p(o["st"]), au=p(buf), off=p(off), coeffs=p(o["coeffs"]), ics=p(o["ics"]), tools=p(o["tools"]), info=p(o["info"]),
                 status=p(o["status"]), taken=p(o["taken"]), hold=p(o["hold"]))
        a.update(null)
        return L.heaac_debug_aac_parse_core_streams(C.byref(cfg), a["st"], a["au"], a["off"], C.c_size_t(S), C.c_size_t(T), cc,
                                                    a["coeffs"], a["ics"], a["tools"], a["info"], a["status"], a["taken"], a["hold"], None)

    def untouched(o):
        return all((v.view(np.uint8) == PC.FILL).all() for v in o.values() if v is not None)

    def refused(f, **kw):
        o = outs()
        assert f(o, **kw) == -1, kw
        assert untouched(o), kw

    for name in ("st", "au", "off", "coeffs", "ics", "tools", "info", "status", "taken"):
        refused(aac, **{name: None})
        refused(he, **{name: None})
    for name in ("sst_in", "sst", "hdr", "sbr", "ps"):
        refused(he, **{name: None})
    for f in (aac, he):
        refused(f, T=0)
        refused(f, cc=0)
        refused(f, cc=3)
        for name in ("coeffs", "tools", "off", "info", "status", "taken"):
            o = outs()
            assert f(o, **{name: C.c_void_p(dict(o, off=off)[name].ctypes.data + 2)}) == -1 and untouched(o), name
        o = outs()
        assert f(o, S=0) == 0 and untouched(o)
        assert f(o, S=0, T=0) == -1
    refused(he, n_hdr=0)
    o = outs()
    assert he(o, sst_in=p(o["sst"])) == -1 and untouched(o)                                   # the state arrays overlap
    assert he(o, sst_in=C.c_void_p(o["sst"].ctypes.data + ch.sst.shape[1])) == -1 and untouched(o)
    for name in ("sst", "hdr", "sbr", "ps"):
        o = outs()
        assert he(o, **{name: C.c_void_p(dict(o, hdr=hdr)[name].ctypes.data + 2)}) == -1 and untouched(o), name
    assert L.heaac_debug_aac_parse_core_streams(None, None, None, None, C.c_size_t(0), C.c_size_t(1), 1, *([None] * 8)) == -1
    big = C.c_size_t(1 << 40)
    o = outs()
    assert aac(o, S=big.value, T=big.value) == -1 and untouched(o)                                # S * T overflows
    assert aac(o, S=1 << 20, T=1 << 13) == -1 and untouched(o)                                     # beyond the 32-bit unit index
    # hold is optional; the good call takes everything
    o = outs()
    o["st"][...] = ch.st
    assert he(o, hold=None) == 0 and (o["taken"] == T).all() and (o["hold"] == PC.FILL).all()


def test_chains_under_sanitizers_with_every_unit_at_the_end_of_its_buffer(pkg):
    """Chains of good, deferred and damaged units through an ASan / UBSan build of the two chains and of the host
    parser (tests/c/fuzz_parse_streams.c), a stand-alone program run as a child: every unit sits at the very end of a
    heap block of exactly its size; the harness checks the three rules itself and counts what it saw."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "fuzz_parse_streams")
    srcs = [os.path.join(ROOT, "tests", "c", "fuzz_parse_streams.c")] + [os.path.join(CSRC, f) for f in (
        "sbr_parse.c", "sbr_header.c", "aac_parse.c", "parse_tables.c")]
    deps = srcs + [os.path.join(CSRC, f) for f in ("parse_streams.h", "sbr_core.h", "parse_core.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + srcs +
                              ["-o", exe, "-lm", "-lpthread"])
    seeds = os.path.join(BUILD, "parse_streams_seeds.bin")
    rng = np.random.default_rng(79)
    with open(seeds, "wb") as f:
        for cpe, ps_modes in SD.STREAMS:
            for w in SD.make_writers(pkg, 5, cpe, ps_modes):
                frames = []
                for t in range(10):
                    crc = bool(rng.integers(0, 2))
                    frames.append(SD.he_au(rng, cpe, SD.writer_frame(rng, w, new_header=t in (4, 7), respec=t == 7, crc=crc), crc))
                frames.append(aac_stop_unit(rng, SD.SI, SD.AOT, cpe, "pulse", None))
                frames.append(aac_stop_unit(rng, SD.SI, SD.AOT, cpe, "second_sce", None))
                f.write(struct.pack("<II", 2 if cpe else 1, len(frames)))
                for au in frames:
                    f.write(struct.pack("<I", len(au)) + au)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, seeds, "1500"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.strip().endswith("ok"), p.stdout[-2000:]
    m = re.search(r"chains (\d+): units taken (\d+), streams stopped (\d+) of which by the SBR half (\d+), second SBR walks over "
                  r"more than one unit (\d+), host refuses the stopping unit (\d+)", p.stdout)
    assert m, p.stdout[-2000:]
    assert int(m.group(2)) > 3000 and int(m.group(3)) > 1000 and int(m.group(4)) > 200 and int(m.group(5)) > 50 and \
        int(m.group(6)) > 300, m.group(0)
