"""The SBR / PS payload walk of heaac_sbr_parse_device on the host (csrc/sbr_core.h through heaac_debug_sbr_parse_core)
against the host parser heaac_heaac_parse_frame_ex, unit by unit from the same state: what it takes comes back byte
for byte, what it does not take is deferred with the state row untouched, and it never says OK where the host call
returns anything but HEAAC_PARSE_OK / HEAAC_PARSE_NO_SBR."""
import copy
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sbr_bitwriter as SW
import sbr_device_common as SD
import test_sbr_parse as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg-heaac_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "c", "_build")


class Chain:
    """n streams of one kind: AAC and SBR states, the host's header table, and one step = the host parser from copies
    of the states, the walk from the same states with the host's info, SD.compare between them; the host's states are
    carried on (it is the host that takes a deferred unit)."""

    def __init__(self, pkg, n, cpe):
        self.pkg, self.n, self.cpe = pkg, n, cpe
        self.cfg = SD.he_cfg(pkg, cpe)
        self.with_ps = not cpe
        self.cc = 2 if cpe else 1
        self.tab = pkg.SbrHeaderTable(64)
        self.st = np.zeros(n, pkg.AAC_STREAM_DT)
        self.sst = pkg.sbr_streams(n)

    def step(self, aus, src=None, n_hdr=None, aac_status=None, carry=True, cfg=None):
        """src: the stream each unit starts from (default: unit i from stream i)."""
        pkg, cfg = self.pkg, cfg or self.cfg
        src = np.arange(self.n) if src is None else np.asarray(src)
        st, before = self.st[src].copy(), self.sst[src].copy()
        hdr = self.tab.headers()[:n_hdr]
        sst_host = before.copy()
        host = SD.host_parse(pkg, cfg, st, sst_host, self.tab, aus, self.cc, self.with_ps)
        status = SD.aac_status_of(host["info"]) if aac_status is None else aac_status
        got = pkg.sbr_parse_core(cfg, before, aus, host["info"], hdr, status, self.with_ps,
                                 out=SD.filled(pkg, before, len(aus), self.with_ps))
        ok = SD.compare(pkg, host, sst_host, before, got)
        assert np.array_equal(got["why"] == 0, ok)
        if carry:
            self.st, self.sst = st, sst_host
        return host, got, ok


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("cpe,ps_modes", [(False, "20"), (False, "34"), (True, None)])
def test_writer_streams_are_taken_whole_behind_their_first_header(pkg, cpe, ps_modes, crc):
    rng = np.random.default_rng(7100 + 10 * cpe + crc + (0 if ps_modes is None else int(ps_modes)))
    n = 16
    ch = Chain(pkg, n, cpe)
    writers = SD.make_writers(pkg, n, cpe, ps_modes)
    coupled, ipdopd, envs = set(), 0, set()
    for step in range(6):
        host, got, ok = ch.step(SD.he_units(rng, writers, cpe, crc=crc))
        assert not host["status"].any(), ("precondition: the host parser takes every unit", host["status"])
        if step == 0:                                             # each stream's first header: the host registers it
            assert not ok.any() and (got["why"] == pkg.SBR_WHY_HEADER).all(), got["why"]
            continue
        assert ok.all(), ("deferred share must be exactly 0", step, np.flatnonzero(~ok), got["why"][~ok])
        assert (got["sbr"]["start"] == 1).all() and (got["sbr"]["reset"] == 0).all()
        coupled |= set(got["sbr"]["bs_coupling"].tolist())
        envs |= set(got["sbr"]["ch"]["bs_num_env"][:, 0].tolist())
        if not cpe:
            ipdopd += int(got["ps"]["enable_ipdopd"].sum())
            assert (got["ps"]["start"] == 1).any()
    assert len(envs) >= 3
    assert coupled == ({0, 1} if cpe else {0})
    assert cpe or ps_modes == "20" or ipdopd > 0                  # 34-band frames carry IPD / OPD


@pytest.mark.parametrize("cpe", [False, True])
def test_a_repeated_header_is_taken_and_a_changed_one_deferred(pkg, cpe):
    rng = np.random.default_rng(7200 + cpe)
    n = 12
    ch = Chain(pkg, n, cpe)
    writers = SD.make_writers(pkg, n, cpe)
    ch.step(SD.he_units(rng, writers, cpe))
    ch.step(SD.he_units(rng, writers, cpe))
    with SD.resent_header("same") as state:                       # the header again, field for field
        aus = SD.he_units(rng, writers, cpe, new_header=True, before=lambda w: state.update(header=w.header))
    before = ch.sst.copy()
    host, got, ok = ch.step(aus)
    assert not host["status"].any() and ok.all(), got["why"]
    assert (got["sbr"]["reset"] == 0).all() and (got["sbr"]["start"] == 1).all()
    assert np.array_equal(got["sst"][:, SD.HDR_AT], before[:, SD.HDR_AT])
    with SD.resent_header("limiter") as state:                    # only a limiter field: another derived record
        aus = SD.he_units(rng, writers, cpe, new_header=True, before=lambda w: state.update(header=w.header))
    before = ch.sst.copy()
    host, got, ok = ch.step(aus)
    assert not host["status"].any() and not ok.any() and (got["why"] == pkg.SBR_WHY_HEADER).all()
    assert (host["sbr"]["reset"] == 0).all() and (ch.sst[:, SD.HDR_AT] != before[:, SD.HDR_AT]).all()
    host, got, ok = ch.step(SD.he_units(rng, writers, cpe))       # and the stream goes on, on the new record
    assert ok.all()
    host, got, ok = ch.step(SD.he_units(rng, writers, cpe, new_header=True, respec=True))       # another spectrum
    assert not host["status"].any() and not ok.any() and (got["why"] == pkg.SBR_WHY_HEADER).all()
    assert (host["sbr"]["reset"] == 1).all()


@pytest.mark.parametrize("cpe", [False, True])
def test_units_without_a_payload_and_streams_with_sbr_off(pkg, cpe):
    rng = np.random.default_rng(7300 + cpe)
    n = 8
    ch = Chain(pkg, n, cpe)
    writers = SD.make_writers(pkg, n, cpe)
    ch.step(SD.he_units(rng, writers, cpe))
    before = ch.sst.copy()
    assert (before[:, SD.KX_AT] != before[:, SD.KX_AT + 1]).all()          # kx[0] = 32 still, kx[1] the header's
    host, got, ok = ch.step([SD.he_au(rng, cpe) for _ in range(n)], carry=False)
    assert (host["status"] == pkg.PARSE_NO_SBR).all() and ok.all()
    assert (got["sbr"]["start"] == 0).all() and (got["sbr"]["hdr"] > 0).all()
    for at in (SD.KX_AT, SD.M_AT):
        assert np.array_equal(got["sst"][:, at], before[:, at + 1]) and np.array_equal(got["sst"][:, at + 1], before[:, at + 1])
    # the same for units WITH a payload where the configuration has no SBR: the payload is not looked at
    off = SD.he_cfg(pkg, cpe)
    off.sbr = 0
    host, got, ok = ch.step(SD.he_units(rng, writers, cpe), carry=False, cfg=off)
    assert (host["info"]["sbr_payload_bit"] > 0).all()
    assert (host["status"] == pkg.PARSE_NO_SBR).all() and ok.all() and (got["sbr"]["start"] == 0).all()
    assert np.array_equal(got["sst"][:, SD.KX_AT], before[:, SD.KX_AT + 1])


def _ps_less_frame_ending_in_the_extension_flag(pkg, rng, w, sst_row, tab):
    """A frame of a writer without PS that ends in bs_extended_data = 0 (test_sbr_parse.py's search)."""
    while True:
        keep = copy.deepcopy((w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling))
        bits, _ = w.frame(rng)
        info = pkg.sbr_parse_payload(sst_row.copy(), tab, 24000, SW.to_bytes(bits), 1, False)[3]
        if bits[-1] == 0 and info["sbr_bits"] == len(bits):
            flipped = pkg.sbr_parse_payload(sst_row.copy(), tab, 24000, SW.to_bytes(bits[:-1] + [1]), 1, False)[3]
            if flipped["sbr_bits"] > len(bits):
                return bits
        w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling = keep


def test_the_other_deferred_classes_leave_the_state_untouched(pkg):
    rng = np.random.default_rng(7400)
    n = 8
    for cpe in (False, True):
        ch = Chain(pkg, n, cpe)
        writers = SD.make_writers(pkg, n, cpe)
        ch.step(SD.he_units(rng, writers, cpe))
        ch.step(SD.he_units(rng, writers, cpe))
        aus = SD.he_units(rng, writers, cpe)
        # the stream's header index is not below n_hdr
        host, got, ok = ch.step(aus, n_hdr=1, carry=False)
        assert not host["status"].any() and not ok.any() and (got["why"] == pkg.SBR_WHY_HDR_INDEX).all()
        # the AAC half did not take the unit: by its status, and for units the host's AAC parser refuses
        host, got, ok = ch.step(aus, aac_status=np.ones(n, np.int32), carry=False)
        assert not ok.any() and (got["why"] == pkg.SBR_WHY_AAC).all()
        host, got, ok = ch.step([au[:3] for au in aus], carry=False)
        assert (host["status"] < 0).all() and not ok.any() and (got["why"] == pkg.SBR_WHY_AAC).all()
        host, got, ok = ch.step(aus, carry=False)                 # (the units themselves are taken)
        assert ok.all()
        # a payload that does not stand directly behind its element (nothing behind its header flag is read)
        aus = [SD.he_au(rng, cpe, SD.writer_frame(rng, w), misplaced=True) for w in writers]
        host, got, ok = ch.step(aus, carry=False)
        assert (host["info"]["sbr_misplaced"] == 1).all() and (host["status"] == -1).all()
        assert not ok.any() and (got["why"] == pkg.SBR_WHY_MISPLACED).all()
        # malformed grids (test_sbr_parse.BAD_GRIDS), in the first and in the second channel of a pair
        for grid in TS.BAD_GRIDS:
            b = SW.Bits()
            b.put(0, 1); b.put(0, 1)                              # no header, no bs_data_extra
            if cpe:
                b.put(0, 1)                                       # not coupled
            for v, k in grid:
                b.put(v, k)
            host, got, ok = ch.step([SD.he_au(rng, cpe, b.bits + [0] * 64) for _ in range(n)], carry=False)
            assert (host["status"] == -1).all() and not ok.any() and (got["why"] == pkg.SBR_WHY_REFUSED).all()
    # illegal PS data (a reserved IID mode) behind a good SBR frame: the host returns the PS reader's error
    ch = Chain(pkg, n, False)
    writers = SD.make_writers(pkg, n, False, ps=False)
    ch.step(SD.he_units(rng, writers, False))
    x = SW.Bits()
    x.put(2, 2)                                                   # EXTENSION_ID_PS
    x.put(1, 1); x.put(1, 1); x.put(7, 3)                         # header, enable_iid, iid_mode 7: reserved
    x.bits.extend([1] * 17)
    cnt = (len(x) + 7) // 8
    size = SW.Bits(); size.put(cnt, 4)
    x.bits.extend([0] * (8 * cnt - len(x)))
    aus = []
    for i, w in enumerate(writers):
        bits = _ps_less_frame_ending_in_the_extension_flag(pkg, rng, w, ch.sst[i], ch.tab)
        aus.append(SD.he_au(rng, False, bits[:-1] + [1] + size.bits + x.bits))
    host, got, ok = ch.step(aus, carry=False)
    assert (host["status"] == -1).all() and (host["sbr"]["start"] == 1).all() and (host["ps"]["start"] == 0).all()
    assert not ok.any() and (got["why"] == pkg.SBR_WHY_REFUSED).all()


@pytest.mark.parametrize("cpe", [False, True])
def test_damaged_units(pkg, cpe):
    """Truncation at every byte of three units, 400 units with 1 - 3 bit flips inside the payload, 200 random payloads
    behind a good core, each from the steady state of a stream: the three rules of SD.compare."""
    rng = np.random.default_rng(7500 + cpe)
    n = 24
    ch = Chain(pkg, n, cpe)
    writers = SD.make_writers(pkg, n, cpe)
    ch.step(SD.he_units(rng, writers, cpe))
    ch.step(SD.he_units(rng, writers, cpe))
    aus = SD.he_units(rng, writers, cpe, crc=True)
    host, _, ok = ch.step(aus, carry=False)
    assert ok.all()
    units, src = SD.damaged(rng, aus, host["info"], cpe=cpe)
    assert len(units) > 600 + 3 * 50
    host, got, ok = ch.step(units, src=src, carry=False)
    print("damaged units %d: ok %d, host refuses %d, why %s" % (len(units), ok.sum(), (host["status"] < 0).sum(),
                                                                 np.unique(got["why"], return_counts=True)))
    assert ok.sum() > 0, "the corpus is all-deferred"


def test_walk_under_sanitizers_with_every_unit_at_the_end_of_its_buffer(pkg):
    """The same damage through an ASan / UBSan build of the walk and of the host parser (tests/c/fuzz_sbr_core.c), a
    stand-alone program run as a child: every unit sits at the very end of a heap block of exactly its size, so a
    read of one byte past the unit is a report; the harness checks the rules itself and counts what it saw."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "fuzz_sbr_core")
    srcs = [os.path.join(ROOT, "tests", "c", "fuzz_sbr_core.c")] + [os.path.join(CSRC, f) for f in (
        "sbr_parse.c", "sbr_header.c", "aac_parse.c", "parse_tables.c")]
    deps = srcs + [os.path.join(CSRC, "sbr_core.h"), os.path.join(CSRC, "parse_core.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + srcs +
                              ["-o", exe, "-lm", "-lpthread"])
    seeds = os.path.join(BUILD, "sbr_core_seeds.bin")
    rng = np.random.default_rng(78)
    with open(seeds, "wb") as f:
        for cpe, ps_modes in SD.STREAMS:
            for w in SD.make_writers(pkg, 6, cpe, ps_modes):
                frames = []
                for t in range(8):
                    crc = bool(rng.integers(0, 2))
                    frames.append(SD.he_au(rng, cpe, SD.writer_frame(rng, w, new_header=t in (3, 6), respec=t == 6, crc=crc), crc))
                f.write(struct.pack("<II", 2 if cpe else 1, len(frames)))
                for au in frames:
                    f.write(struct.pack("<I", len(au)) + au)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, seeds, "200"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-4000:]
    assert p.stdout.strip().endswith("ok"), p.stdout[-2000:]
    m = re.search(r"units (\d+): walk ok (\d+), deferred (\d+) of which the host parser takes (\d+), refuses (\d+)", p.stdout)
    assert int(m.group(2)) > 2000 and int(m.group(5)) > 2000 and int(m.group(4)) >= 24, m.group(0)


TAKEN = ("plain", "same_header", "no_payload")
DAMAGE = ("flipped", "truncated")


@pytest.mark.parametrize("cpe", [False, True])
def test_all_classes_mixed_in_one_call(pkg, cpe):
    """The corpus of the GPU tests (SD.mixed_units) on the host first: every class lands where the contract puts it."""
    rng = np.random.default_rng(7600 + cpe)
    n = 65
    ch = Chain(pkg, n, cpe)
    writers = SD.make_writers(pkg, n, cpe)
    ch.step(SD.he_units(rng, writers, cpe))
    seen = set()
    in_step = np.ones(n, bool)             # the decoder still holds what the stream's writer thinks it holds
    for step in range(3):
        classes = [SD.CLASSES[int(k)] for k in rng.integers(0, len(SD.CLASSES), n)]
        host, got, ok = ch.step(SD.mixed_units(rng, writers, cpe, classes))
        for i, cls in enumerate(classes):
            if cls not in DAMAGE and in_step[i]:
                assert ok[i] == (cls in TAKEN), (step, i, cls, got["why"][i], host["status"][i])
                seen.add((cls, bool(ok[i])))
            # a misplaced payload or a bad grid stops the stream, damage may have been taken for data: from there on
            # only the rules of SD.compare are asked of that stream
            in_step[i] &= cls not in DAMAGE + ("misplaced", "bad_grid")
    assert {(c, c in TAKEN) for c in SD.CLASSES if c not in DAMAGE} <= seen
