"""Mint tests/golden/sbr_error_states.json: what heaac_sbr_parse_payload leaves behind for a payload it refuses -- status,
HeaacSbrParseInfo, both records and the HeaacSbrStream row (as its difference from the row in front of the unit) --
and the records of the next good frame of the stream, which reads what the error left (num_env_old, the rows time
deltas continue from, is34bands, the rolled-back channels).  tests/test_sbr_parse_error_state.py replays the bytes.

The fixture pins the behaviour of the host parser AS IT WAS when csrc/sbr_parse.c still held readers of its own: it is
minted against a build of commit 63469a7 (the parent of the change that made csrc/sbr_core.h the one writing), never
against the tree it is then used to test:

    HEAAC_LIB_PATH=<build of 63469a7>/ffmpeg-heaac_amd/libheaac_amd.so python tests/golden/make_sbr_error_states.py

Every case starts from a stream of tests/sbr_bitwriter.py two good frames in.  The cases: one crafted payload per exit
of the Parametric Stereo reader (csrc/sbr_core.h: sc_ps), each of test_sbr_parse.BAD_GRIDS in an SCE and in the second
channel of an uncoupled CPE, an envelope value pushed above 255, a truncated unit.  One exit of the PS reader has no
case: "a prefix that is no code" cannot be written, since all twenty code books are complete (Kraft sum 1; the generator
checks it) and the bit reader yields zeros past the end of a unit, so every prefix is a code.
"""
import importlib, json, os, sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PARENT = "63469a7"
OUT = os.path.join(ROOT, "tests", "golden", "sbr_error_states.json")
ERR_DATA, ERR_OVERREAD = -1, -2


def parse(pkg, st, tab, payload, channels, allow_ps):
    return pkg.sbr_parse_payload(st[0], tab, 24000, payload, channels, allow_ps)


def diff_runs(before, after):
    """[[offset, hex of the bytes of `after`], ...] for every run of bytes that differ."""
    at = np.flatnonzero(before != after)
    runs = []
    for k in at:
        if runs and k == runs[-1][0] + len(runs[-1][1]):
            runs[-1][1].append(int(after[k]))
        else:
            runs.append([int(k), [int(after[k])]])
    return [[o, bytes(v).hex()] for o, v in runs]


def body_ending_in_the_extension_flag(pkg, SW, SD, rng, w, st, tab):
    """A frame of the writer without its PS data whose last bit is bs_extended_data = 0, that bit taken off."""
    ps, w.ps = w.ps, None
    try:
        while True:
            keep = SD.snapshot(w)
            bits, _ = w.frame(rng)
            info = parse(pkg, st.copy(), tab, SW.to_bytes(bits), 1, False)[3]
            if bits[-1] == 0 and info["sbr_bits"] == len(bits):
                flipped = parse(pkg, st.copy(), tab, SW.to_bytes(bits[:-1] + [1]), 1, False)[3]
                if flipped["sbr_bits"] > len(bits):
                    return bits[:-1]
            SD.restore(w, keep)
    finally:
        w.ps = ps


def extended(SW, body, ps_bits, cnt=None):
    """body, bs_extended_data = 1, the size, EXTENSION_ID_PS and ps_bits; cnt: the byte count sent (default: what fits)."""
    x = SW.Bits(); x.put(2, 2); x.bits.extend(ps_bits)
    n = (len(x) + 7) // 8 if cnt is None else cnt
    b = SW.Bits(); b.bits = list(body); b.put(1, 1)
    if n >= 15:
        b.put(15, 4); b.put(n - 15, 8)
    else:
        b.put(n, 4)
    b.bits.extend(x.bits)
    b.bits.extend([0] * max(0, 8 * n - len(x)))
    return b.bits


def ps_data(SW, iid=None, icc=None, ext=0, cls=0, idx=1, borders=()):
    """ps_data() up to its time grid, with a header: iid / icc = the mode of a kind that is on."""
    b = SW.Bits()
    b.put(1, 1)
    for mode in (iid, icc):
        b.put(int(mode is not None), 1)
        if mode is not None:
            b.put(mode, 3)
    b.put(ext, 1)
    b.put(cls, 1); b.put(idx, 2)
    for x in borders:
        b.put(x, 5)
    return b


def along_frequency(SW, b, table, values):
    b.put(0, 1)
    last = 0
    for v in values:
        b.huff(table, v - last + SW.T["ps_offset"][table])
        last = v


def ps_cases(SW):
    """name -> (set-up PS frames that must parse, the refused ps_data(), byte count sent or None, status)"""
    cases = {}
    b = SW.Bits(); b.put(1, 1); b.put(1, 1); b.put(7, 3); b.bits.extend([1] * 17)
    cases["ps_reserved_iid_mode"] = ([], b.bits, None, ERR_DATA)
    b = SW.Bits(); b.put(1, 1); b.put(1, 1); b.put(1, 3); b.put(1, 1); b.put(6, 3); b.bits.extend([1] * 17)
    cases["ps_reserved_icc_mode"] = ([], b.bits, None, ERR_DATA)
    b = ps_data(SW, iid=0)
    along_frequency(SW, b, "iid_df0", [7, 14]); b.bits.extend([0] * 24)           # coarse quantiser: |iid| <= 7
    cases["ps_iid_value_out_of_range"] = ([], b.bits, None, ERR_DATA)
    b = ps_data(SW, icc=0)
    along_frequency(SW, b, "icc_df", [7, 8]); b.bits.extend([0] * 24)
    cases["ps_icc_value_out_of_range"] = ([], b.bits, None, ERR_DATA)
    b = ps_data(SW, iid=1, ext=1, idx=2)                                          # two envelopes, 11 phases each
    for e in range(2):
        along_frequency(SW, b, "iid_df0", [0] * 20)
    b.put(1, 4)                                                                   # one byte of extensions ...
    b.put(0, 2); b.put(1, 1)                                                      # ... and IPD / OPD that need more
    for e in range(2):
        along_frequency(SW, b, "ipd_df", [e + 1] * 11)
        along_frequency(SW, b, "opd_df", [e + 2] * 11)
    b.put(0, 1)
    cases["ps_extensions_past_their_count"] = ([], b.bits, None, ERR_DATA)
    b = ps_data(SW, cls=1, idx=1, borders=(10, 5))
    cases["ps_borders_not_ascending"] = ([], b.bits, None, ERR_DATA)
    fine = ps_data(SW, iid=3)                                                     # fine quantiser, 10 bands, all 12
    along_frequency(SW, fine, "iid_df1", [12] * 10)
    b = ps_data(SW, iid=0, idx=0)                                                 # coarse, no envelope: borrows the 12s
    cases["ps_borrowed_value_outside_the_quantiser"] = ([fine.bits], b.bits, None, ERR_DATA)
    b = ps_data(SW, iid=0)
    along_frequency(SW, b, "iid_df0", [3] * 10)
    cases["ps_longer_than_its_extension"] = ([], b.bits, 1, ERR_OVERREAD)
    return cases


def main():
    pkg = importlib.import_module("ffmpeg-heaac_amd")
    import sbr_bitwriter as SW
    import sbr_device_common as SD
    import test_sbr_parse as TS
    for name in SW.SBR_T + SW.PS_T:
        assert sum(Fraction(1, 2 ** int(n)) for n in SW.T[name][1]) == 1, (name, "is not a complete code")
    out = []

    def start(seed, channels, ps):
        """A stream two good frames in (with PS: both kinds of frame have started)."""
        while True:
            rng = np.random.default_rng(seed)
            w = SW.SbrStreamWriter(pkg, channels, ps=ps, varfrac=0.6)
            tab, st, setup = pkg.SbrHeaderTable(8), pkg.sbr_streams(1), []
            for _ in range(2):
                setup.append(SW.to_bytes(w.frame(rng)[0]))
                r, sbr, psr, _ = parse(pkg, st, tab, setup[-1], channels, ps)
                assert r == 0
            if not ps or (psr["start"][0] == 1 and psr["num_env"][0] > 1):
                return rng, w, tab, st, setup
            seed += 1000

    def finish(name, rng, w, tab, st, setup, channels, ps, unit, status, next_header):
        before = st.copy()
        r, sbr, psr, info = parse(pkg, st, tab, unit, channels, ps)
        assert r < 0 and status in (None, r), (name, r, info)
        expect = dict(status=int(r), info=[int(info[k]) for k in ("sbr_bits", "header", "ps_present", "ps_status")],
                      sbr=sbr.tobytes().hex(), ps=psr.tobytes().hex(), state_diff=diff_runs(before[0], st[0]))
        # the next good frame, preferably one the parser takes whole (the writer does not know what the error left)
        keep, row = SD.snapshot(w), st.copy()
        for attempt in range(64):
            if ps:
                w.ps.start = 0                                                    # as the decoder: the next PS frame brings a header
            payload = SW.to_bytes(w.frame(rng, new_header=next_header)[0])
            st[...] = row
            r2, sbr2, psr2, _ = parse(pkg, st, tab, payload, channels, ps)
            if r2 == 0 and sbr2["start"][0] == 1 and (not ps or psr2["start"][0] == 1):
                break
            SD.restore(w, keep)
        out.append(dict(name=name, channels=channels, allow_ps=int(ps), setup=[p.hex() for p in setup], unit=unit.hex(), expect=expect,
                        next=dict(payload=payload.hex(), status=int(r2), sbr=sbr2.tobytes().hex(), ps=psr2.tobytes().hex())))
        print("%-44s status %2d info %s, %3d state bytes moved; next frame: status %d, sbr.start %d, ps.start %d" % (
            name, r, expect["info"], sum(len(h) // 2 for _, h in expect["state_diff"]), r2, sbr2["start"][0], psr2["start"][0]))
        return info, sbr, psr

    # ---- the exits of the PS reader: the SBR frame stands, PS is switched off ----
    for k, (name, (pre, ps_bits, cnt, status)) in enumerate(ps_cases(SW).items()):
        rng, w, tab, st, setup = start(100 + k, 1, True)
        for bits in pre:
            setup.append(SW.to_bytes(extended(SW, body_ending_in_the_extension_flag(pkg, SW, SD, rng, w, st, tab), bits)))
            r, _, psr, _ = parse(pkg, st, tab, setup[-1], 1, True)
            assert r == 0 and psr["start"][0] == 1, name
        unit = extended(SW, body_ending_in_the_extension_flag(pkg, SW, SD, rng, w, st, tab), ps_bits, cnt)
        info, sbr, psr = finish(name, rng, w, tab, st, setup, 1, True, SW.to_bytes(unit), status, False)
        assert info["ps_present"] == 1 and info["ps_status"] == status and sbr["start"][0] == 1 and psr["start"][0] == 0, name

    # ---- refused elements: the channels are rolled back, SBR is off until the next header ----
    for cpe in (False, True):
        for g, grid in enumerate(TS.BAD_GRIDS):
            rng, w, tab, st, setup = start(200 + 10 * cpe + g, 2 if cpe else 1, not cpe)
            b = SW.Bits()
            b.put(0, 1); b.put(0, 1)                                              # no header, no bs_data_extra
            if cpe:
                b.put(0, 1)                                                       # not coupled
                b.put(0, 2); b.put(0, 2); b.put(1, 1)                             # first channel: FIXFIX, one envelope
            for v, n in grid:
                b.put(v, n)
            info, sbr, _ = finish("bad_grid_%d_in_%s" % (g, "the_second_channel_of_a_cpe" if cpe else "an_sce"), rng, w, tab, st, setup,
                                  2 if cpe else 1, not cpe, SW.to_bytes(b.bits, 64), ERR_DATA, True)
            assert sbr["start"][0] == 0
    rng, w, tab, st, setup = start(300, 1, True)
    n, n_q = int(w.hdr_rec[0]["n"][1]), int(w.hdr_rec[0]["n_q"])
    lav = int(SW.T["sbr_lav"]["f_env_15"])
    assert n >= 4 and 127 + 3 * lav > 255
    b = SW.Bits()
    b.put(0, 1); b.put(0, 1)
    b.put(0, 2); b.put(0, 2); b.put(1, 1)                                         # FIXFIX, one envelope (so 1.5 dB steps), high resolution
    b.put(0, 1); b.put(0, 1)                                                      # both along frequency
    for _ in range(n_q):
        b.put(0, 2)
    b.put(127, 7)
    for j in range(1, n):
        b.sbr("f_env_15", lav if j <= 3 else 0)                                   # 127 + 3 lav > 255
    b.put(0, 5)
    for j in range(1, n_q):
        b.sbr("f_env_30", 0)
    b.put(0, 1); b.put(0, 1)                                                      # no harmonics, no extended data
    info, sbr, _ = finish("envelope_value_above_255", rng, w, tab, st, setup, 1, True, SW.to_bytes(b.bits), ERR_DATA, True)
    assert info["sbr_bits"] == len(b.bits) - 1 and sbr["start"][0] == 0        # the whole element was read, up to the flag behind it: only the range is wrong
    rng, w, tab, st, setup = start(301, 1, True)
    keep = SD.snapshot(w)
    bits = w.frame(rng)[0]
    SD.restore(w, keep)
    finish("truncated_unit", rng, w, tab, st, setup, 1, True, SW.to_bytes(bits[:len(bits) // 16 * 8], pad=0), None, True)

    about = ("What heaac_sbr_parse_payload of commit %s leaves behind refused payloads; minted by tests/golden/make_sbr_error_states.py "
             "against a build of that commit, replayed by tests/test_sbr_parse_error_state.py.  Payloads and records are hex; state_diff "
             "is [[offset, bytes], ...] of the HeaacSbrStream row against the row in front of the unit." % PARENT)
    with open(OUT, "w") as f:
        json.dump(dict(about=about, minted_against=PARENT, cases=out), f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
