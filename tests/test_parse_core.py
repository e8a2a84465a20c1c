"""The access-unit walk of heaac_aac_parse_device on the host (csrc/parse_core.h through heaac_debug_aac_parse_core)
against the host parser heaac_aac_parse_frame_ex, unit by unit: what it takes comes back byte for byte, what it does
not take is deferred with the stream state untouched, and it never says OK where the host parser refuses.

Both read the element syntax through the same pc_* readers of csrc/parse_core.h, so this is not one writing of the
syntax checked by another: it pins the walk's defer mode (no PcHost record, every failure gives the unit up, the
state committed on OK only) against the host's refuse mode of the same readers, the element loop pc_walk against
frame_walk, and the bounds.  The independent statement of the values is the bit writer (test_parse.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import parse_device_common as PC
import test_parse as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg-heaac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")
# the cases of test_parse.py::test_written_access_units_come_back, plus a mono AAC-Main one
CASES = [(False, 2, 3), (True, 2, 3), (True, 1, 4), (False, 2, 6), (True, 2, 11), (False, 1, 4)]


def core(pkg, cfg, st, aus, cc):
    out = PC.filled(pkg, len(aus), cc)
    return pkg.aac_parse_core(cfg, st, aus, coeff_channels=cc, out=out)


def run(pkg, cfg, st, aus, cc):
    """One call of the core on `st` (updated in place) compared with the host parser; returns (host status, ok, why)."""
    before = st.copy()
    got = core(pkg, cfg, st, aus, cc)
    host, ok = PC.compare(pkg, cfg, before, aus, cc, got, st)
    assert np.array_equal(got["why"] == 0, ok)
    return host, ok, got["why"]


@pytest.mark.parametrize("cpe,aot,si", CASES)
@pytest.mark.parametrize("adts", [0.0, 1.0])
def test_in_scope_units_come_back_as_the_host_parser_writes_them(pkg, cpe, aot, si, adts):
    rng = np.random.default_rng(2200 + 7 * si + cpe + 100 * aot + int(adts))
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    n, steps = 40, 4
    for cc in ((2,) if cpe else (1, 2)):
        st = np.zeros(n, pkg.AAC_STREAM_DT)
        for aus in PC.in_scope_steps(rng, si, aot, cpe, n, steps, adts=adts, sbr=0.3):
            host, ok, why = run(pkg, cfg, st, aus, cc)
            assert not host.any(), ("precondition: the host parser takes the whole corpus", host)
            assert ok.all(), ("deferred in-scope units", np.flatnonzero(~ok), why[~ok])
        assert st["oc"].all() and st["mapped_tag"].all()      # the chain has moved the configuration state


def test_main_profile_tns_up_to_order_20(pkg):
    rng = np.random.default_rng(2020)
    cfg = TP._cfg(pkg, 1, 4, 1)
    units = PC.main_high_order_units(rng, 4, 24)
    aus = [u for u, _ in units]
    st = np.zeros(len(aus), pkg.AAC_STREAM_DT)
    before = st.copy()
    got = core(pkg, cfg, st, aus, 1)
    host, ok = PC.compare(pkg, cfg, before, aus, 1, got, st)
    assert not host.any() and ok.all(), (host, got["why"])
    assert sorted(set(int(t["ch"][0]["tns"]["order"][0][0]) for t in got["tools"])) == list(range(13, 21))
    assert [int(t["ch"][0]["tns"]["order"][0][0]) for t in got["tools"]] == [o for _, o in units]
    # the same units are refused in an AAC-LC stream (order > 12): deferred, by the host parser's own check
    lc = TP._cfg(pkg, 2, 4, 1)
    st = np.zeros(len(aus), pkg.AAC_STREAM_DT)
    got = core(pkg, lc, st, aus, 1)
    host, ok = PC.compare(pkg, lc, st.copy(), aus, 1, got, st)
    assert host.all() and not ok.any()


def test_implicit_ps_and_tag_state_follow_the_host_parser(pkg):
    """A mono stream with implicit SBR / PS: the first SBR payload re-configures the output (the mapped tag is
    forgotten) until a unit locks it; units behind ADTS headers reset it again before the lock."""
    rng = np.random.default_rng(31)
    cfg = TP._cfg(pkg, 2, 6, 1)
    cfg.sbr, cfg.ps = -1, -1
    n = 24
    st = np.zeros(n, pkg.AAC_STREAM_DT)
    for aus in PC.in_scope_steps(rng, 6, 2, False, n, 3, adts=0.5, sbr=0.7):
        host, ok, _ = run(pkg, cfg, st, aus, 1)
        assert not host.any() and ok.all()


@pytest.mark.parametrize("cpe,aot,si", [(False, 2, 3), (True, 2, 3), (True, 1, 4)])
def test_out_of_scope_units_are_deferred_with_the_state_untouched(pkg, cpe, aot, si):
    rng = np.random.default_rng(4300 + cpe + aot)
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    aus = PC.deferred_units(rng, si, aot, cpe, 24)
    st = np.zeros(len(aus), pkg.AAC_STREAM_DT)
    st["window_sequence"] = rng.integers(0, 4, (len(aus), 2))
    st["mapped_tag"][::2] = 1
    st["oc"][::3] = 1
    host, ok, why = run(pkg, cfg, st, aus, 2)
    assert not ok.any(), np.flatnonzero(ok)
    assert (host[:24] == 0).all() and (why[:24] == pkg.PARSE_WHY_PULSE).all()         # pulse data parses on the host
    assert (host == 0).sum() > 24                                                      # so do program config elements
    for i in np.flatnonzero(host == 0):                                                 # the classes, read independently
        c = PC.classify(aus[i], si, aot)
        assert c is None or why[i] == (pkg.PARSE_WHY_PULSE if c == "pulse" else pkg.PARSE_WHY_ELEMENT), (i, c, why[i])
    # not vacuous: of the 24 pulse units about half carry the pulse data in the first channel, and 8 of the 24 wide
    # units open with a program config element -- some 20 are expected to be confirmed; ask for half of that
    assert sum(PC.classify(aus[i], si, aot) is not None for i in np.flatnonzero(host == 0)) >= 10
    assert set(why[host == 0]) == {pkg.PARSE_WHY_PULSE, pkg.PARSE_WHY_ELEMENT}


@pytest.mark.parametrize("cpe,aot,si", [(False, 2, 3), (True, 2, 3), (True, 1, 4)])
def test_damaged_units(pkg, cpe, aot, si):
    """core OK => host OK with identical records and state; host not OK => DEFERRED, state untouched (both in
    PC.compare); host OK and DEFERRED only for the deferred classes."""
    rng = np.random.default_rng(5100 + cpe + aot)
    cfg = TP._cfg(pkg, aot, si, 2 if cpe else 1)
    good = [au for row in PC.in_scope_steps(rng, si, aot, cpe, 12, 1, adts=0.4, sbr=0.3) for au in row]
    good += PC.deferred_units(rng, si, aot, cpe, 4)
    aus = PC.damaged_units(rng, good) + PC.written_refusals(rng, si, aot, cpe)
    st = np.zeros(len(aus), pkg.AAC_STREAM_DT)
    st["window_sequence"] = rng.integers(0, 4, (len(aus), 2))
    st["mapped_tag"] = rng.integers(0, 3, len(aus))
    st["oc"] = rng.choice([0, 1, 2, 4, 8, 12], len(aus))
    host, ok, why = run(pkg, cfg, st, aus, 2)
    wrongly = (host == 0) & ~ok & (why == pkg.PARSE_WHY_REFUSED)
    assert not wrongly.any(), ("deferred as refused, but the host parser takes them", np.flatnonzero(wrongly)[:8])
    # the class of every unit the host parser takes, read from the unit's bits by PC.classify and not from the walk's
    # own report: what the walk took is of no deferred class as far as classify follows it, and what it deferred is
    # confirmed there where classify can follow (the rest carry their pulse data or extra element behind the first channel)
    seen = {True: 0, False: 0}
    for i in np.flatnonzero(host == 0):
        c = PC.classify(aus[i], si, aot)
        if ok[i]:
            assert c is None, (i, c)
        else:
            seen[c is not None] += 1
            assert c is None or why[i] == (pkg.PARSE_WHY_PULSE if c == "pulse" else pkg.PARSE_WHY_ELEMENT), (i, c, why[i])
    assert seen[True] >= 10, seen
    # not vacuous: damage that still parses, damage that does not, both in numbers
    assert ok.sum() > 50 and (host != 0).sum() > 200, (ok.sum(), (host != 0).sum())


def test_arguments(pkg):
    cfg = TP._cfg(pkg, 2, 3, 2)
    st = np.zeros(1, pkg.AAC_STREAM_DT)
    au = [b"\x21\x00\x00"]
    for bad in ("aot", "si_hi", "si_lo", "cc0", "cc3"):
        c = TP._cfg(pkg, 2, 3, 2)
        cc = 2
        if bad == "aot":
            c.object_type = 5
        elif bad == "si_hi":
            c.sampling_index = 13
        elif bad == "si_lo":
            c.sampling_index = -1
        else:
            cc = 0 if bad == "cc0" else 3
        with pytest.raises(pkg.HeaacError):
            pkg.aac_parse_core(c, st, au, coeff_channels=cc, out=PC.filled(pkg, 1, 2))
    assert pkg.lib().heaac_debug_aac_parse_core(None, None, None, None, 0, 2, None, None, None, None, None, None) == -1
    import ctypes as C
    assert pkg.lib().heaac_debug_aac_parse_core(C.byref(cfg), None, None, None, C.c_size_t(0), 2, None, None, None, None, None, None) == 0
    assert pkg.lib().heaac_debug_aac_parse_core(C.byref(cfg), None, None, None, C.c_size_t(1), 2, None, None, None, None, None, None) == -1
    # an empty unit and offsets that run backwards are deferred, nothing is read
    off = np.array([4, 4, 2], np.uint32)
    out = PC.filled(pkg, 2, 2)
    status = np.full(2, 7, np.int32)
    st = np.zeros(2, pkg.AAC_STREAM_DT)
    buf = np.zeros(8, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().heaac_debug_aac_parse_core(C.byref(cfg), p(st), p(buf), p(off), C.c_size_t(2), 2, p(out["coeffs"]), p(out["ics"]),
                                              p(out["tools"]), p(out["info"]), p(status), None)
    assert rc == 0 and list(status) == [pkg.PARSE_DEFERRED] * 2


def test_walk_under_sanitizers_with_every_unit_at_the_end_of_its_buffer(pkg):
    """The same damage through an ASan / UBSan build of the walk and of the host parser (tests/c/fuzz_parse_core.c):
    every unit is copied to the very end of a heap block of exactly its size, so a read of one byte past the unit is
    a report; the harness checks the three rules itself and counts what it saw."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "fuzz_parse_core")
    srcs = [os.path.join(ROOT, "tests", "c", "fuzz_parse_core.c")] + [os.path.join(CSRC, f) for f in ("aac_parse.c", "parse_tables.c")]
    deps = srcs + [os.path.join(CSRC, "parse_core.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + srcs +
                              ["-o", exe, "-lm", "-lpthread"])
    seeds = os.path.join(BUILD, "core_seeds.bin")
    rng = np.random.default_rng(77)
    with open(seeds, "wb") as f:
        for cpe, aot, si in [(False, 2, 3), (True, 2, 3), (True, 1, 4)]:
            good = [au for row in PC.in_scope_steps(rng, si, aot, cpe, 10, 1, adts=0.4, sbr=0.3) for au in row]
            good += PC.deferred_units(rng, si, aot, cpe, 3)
            for au in good + PC.damaged_units(rng, good, flips=300, randoms=150) + PC.written_refusals(rng, si, aot, cpe):
                f.write(struct.pack("<IIII", aot, si, 2 if cpe else 1, len(au)) + au)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, seeds, "60000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.strip().endswith("ok"), p.stdout[-2000:]
    import re
    m = re.search(r"units (\d+): core ok (\d+), deferred (\d+) of which the host parser takes (\d+), refuses (\d+)", p.stdout)
    assert int(m.group(2)) > 2000 and int(m.group(5)) > 5000 and int(m.group(4)) > 100, m.group(0)
