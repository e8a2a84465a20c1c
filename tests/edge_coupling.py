"""Records for the multichannel back end (tests/test_coupling_reach.py, tests/test_coupling_grid_gpu.py): dependent
coupling inside the spectral tools, independent coupling behind the IMDCT, and the int16 interleave of any layout.

Host logic only (numpy), generators of its own, one fixed seed.  tests/test_coupling_gpu.py draws its coupling
elements through the bit writer: one sampling index, one or two elements with one or two links, gains of one
magnitude.  This module writes HeaacCceFrame and target HeaacToolsFrame records DIRECTLY and walks the rest of what
the records can hold.  The band tables are those of tests/edge_tools.py (all 13 sampling indices, long and short);
the synth and its draws are not touched.

Every record stays inside what csrc/aac_parse.c can write: offsets from a real table, group_len summing to the
window count, num_window_groups * max_sfb <= 120, n_links <= 4, target_ch in {0, 1}.  The oracle, like the
reference, has no guard; the kernel's clamps for foreign records (n_links, idx < 120, line < 1024) are NOT the
subject of these records and no test built on them says anything about those clamps.

Dependent coupling: units(pkg, profile) gives one batch per profile,
  tables       the coupling channel on the long and short table of every sampling index, max_sfb 0, 1, num_swb - 1 and
               num_swb, the target on the same and on the OTHER window length
  groupings    all 128 groupings of eight short windows on the 15-, 14- and 12-band tables with max_sfb = num_swb
               (grouping 0 on 15 bands walks the gain list to index 119)
  links        n_links 0 .. 4, all 16 target_ch patterns of four links, links that name channel 1 alone (skipped for a
               mono target), one channel twice with different lists
  slots        1, 2, 15 and 16 present slots of HEAAC_MAX_CCE, gaps between them, AFTER_IMDCT slots in between (the
               tools call must leave those alone: their gains and spectra are NaN), both spectral points in one unit
  order        gains chosen so that float addition does not associate: consecutive contributions to a line differ by
               2^+-12 .. 2^+-24 and alternate in sign (order_property asserts that every swap of two contributions
               changes a line)
  zero_bands   band_type all zero, all non-zero, first band only, last band only, alternating; the gains under ZERO
               bands are NaN and must never be read
  gains        every value of tests/golden/cce_gains.json as a band gain, the largest and the smallest side by side
               (+-inf are among them: the one profile whose results are not all finite; one contribution per line,
               no TNS, so that no NaN arises)
  around_tns   targets with one TNS filter per window of order 20, 12 and 7 (the kernel's three order templates) in
               both directions over every band, a BEFORE_TNS and a BETWEEN_TNS_AND_IMDCT element on the same bands,
               M/S, intensity and noise bands on the target

Spectra are standard normal at the level of the tools tests (1024 SF_SCALE).

Independent coupling: couple_case(...) gives heaac_couple_after_imdct_batch records whose sums land on, just inside
and just outside both int16 limits.  Interleave: interleave_pool(sse2) gives the values of each conversion's edges.
"""
import json
import os

import numpy as np

import edge_tools as E

PROFILES = ("tables", "groupings", "links", "slots", "order", "zero_bands", "gains", "around_tns")
FORMS = ("all", "pre_post", "post")          # TOOLS_ALL / TOOLS_PRE then TOOLS_POST / TOOLS_POST alone
SEED = 20240923
MAX_CCE, MAX_LINKS = 16, 4
BEFORE_TNS, BETWEEN, AFTER_IMDCT = 0, 1, 3
LEVEL = np.float32(1024 * E.SF_SCALE)
N_CCE = dict(tables=2, groupings=1, links=2, slots=16, order=16, zero_bands=2, gains=1, around_tns=2)
TNS_TEMPLATE_ORDERS = (20, 12, 7)
SLOT_COUNTS = (1, 2, 15, 16)
BIAS = np.float32(385.0)

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cce_gains.json")) as _f:
    _g = json.load(_f)
GOLDEN = np.array(_g["positive"] + _g["negative"], np.uint32).view(np.float32)     # [8][257]
GOLDEN.setflags(write=False)


def golden_words():
    """the set of all golden gains as uint32 words"""
    return set(int(x) for x in GOLDEN.view(np.uint32).ravel())


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------
def _gains(rng):
    """120 gains as a coupling element of gain_element_scale 0 transmits them: 2^(-step / 8), |step| <= 24, a third
    of them negative"""
    step = rng.integers(-24, 25, 120)
    return GOLDEN[np.where(rng.random(120) < 0.33, 4, 0), 128 + step].copy()


def _band_types(rng, nb, zero=0.15):
    bt = np.zeros(128, np.uint8)
    bt[:nb] = rng.integers(1, 12, nb)
    bt[:nb][rng.random(nb) < zero] = 0
    return bt


def _cce(rec, si, eight, max_sfb, lens, point, links, tag=0, band_type=None, rng=None):
    """one present coupling element: links = [(target_ch, gain[120])]"""
    assert len(links) <= MAX_LINKS
    rec["present"] = 1
    rec["elem_id"] = tag
    rec["coupling_point"] = point
    rec["n_links"] = len(links)
    E._set_ics(rec["ics"], si, eight, max_sfb, lens if eight else None)
    nb = int(rec["ics"]["num_window_groups"]) * max_sfb
    assert nb <= 120
    rec["band_type"] = _band_types(rng, nb) if band_type is None else band_type
    assert not rec["band_type"][nb:].any()
    for l, (ch, gain) in enumerate(links):
        assert ch in (0, 1)
        rec["link"][l]["target_ch"] = ch
        rec["link"][l]["gain"] = gain


def _target(rng, fr, si, eight, max_sfb=None, lens=None, common=True, tns=0.5):
    """a target element with the tools tests' band mix; channel 1 on channel 0's window when common"""
    nswb = len(E.table(si, eight)[0]) - 1
    E._stereo(rng, fr, int(common))
    E._set_ics(fr["ch"][0]["ics"], si, eight, nswb if max_sfb is None else max_sfb,
               (lens or E._random_lens(rng)) if eight else None)
    if common:
        fr["ch"][1]["ics"] = fr["ch"][0]["ics"]
    else:
        other = len(E.table(si, not eight)[0]) - 1
        E._set_ics(fr["ch"][1]["ics"], si, not eight, other, None if eight else E._random_lens(rng))
    for c in range(2):
        ch = fr["ch"][c]
        E._mixed_bands(rng, ch, c)
        E._random_pred(rng, ch, si)
        if tns:
            E._random_tns(rng, ch, tns)


class _Batch:
    def __init__(self, pkg, n, n_cce):
        self.tools = np.zeros(n, pkg.TOOLS_FRAME_DT)
        self.cce = np.zeros((n, n_cce), pkg.CCE_FRAME_DT)
        self.poison = np.zeros((n, n_cce), bool)       # slots whose spectrum is NaN (absent / AFTER_IMDCT)


def _tables(rng, pkg):
    cases = [(si, eight, k, same) for si in range(E.NUM_SI) for eight in (False, True) for k in range(4)
             for same in (True, False)]
    b = _Batch(pkg, len(cases), 2)
    for u, (si, eight, k, same) in enumerate(cases):
        nswb = len(E.table(si, eight)[0]) - 1
        m = (0, 1, nswb - 1, nswb)[k]
        _target(rng, b.tools[u], si, eight if same else not eight, common=u % 3 != 0)
        for s in range(2):
            links = [(s, _gains(rng)), (1 - s, _gains(rng))]
            _cce(b.cce[u, s], si, eight, m, E._random_lens(rng), (BEFORE_TNS, BETWEEN)[s], links, tag=3 + 6 * s, rng=rng)
    return b


def _groupings(rng, pkg):
    classes = sorted(E.SHORT_CLASSES, reverse=True)              # 15, 14, 12
    b = _Batch(pkg, 3 * 128, 1)
    for u in range(3 * 128):
        nswb, bits = classes[u // 128], u % 128
        sis = E.SHORT_CLASSES[nswb]
        si = sis[bits % len(sis)]
        # the target: another grouping of eight short windows two times in three, a long window otherwise
        if bits % 3:
            _target(rng, b.tools[u], si, True, lens=E.grouping_lens((bits * 37 + 11) % 128))
        else:
            _target(rng, b.tools[u], si, False)
        lens = E.grouping_lens(bits)
        bt = _band_types(rng, len(lens) * nswb, zero=0.0 if bits == 0 else 0.15)
        _cce(b.cce[u, 0], si, True, nswb, lens, bits & 1, [(0, _gains(rng)), (1, _gains(rng))], tag=bits % 16,
             band_type=bt)
    return b


LINK_CASES = ([("count", [0, 1, 0, 1][:k]) for k in range(5)] +
              [("pattern", [(p >> 3) & 1, (p >> 2) & 1, (p >> 1) & 1, p & 1]) for p in range(16)] +
              [("mono_skips", [1]), ("mono_skips", [1, 1]), ("twice", [0, 0]), ("twice", [1, 0, 0])])


def _links(rng, pkg):
    b = _Batch(pkg, 2 * len(LINK_CASES), 2)
    for u in range(len(b.tools)):
        kind, chans = LINK_CASES[u % len(LINK_CASES)]
        eight = u >= len(LINK_CASES)
        si = (3, 8)[u % 2]
        _target(rng, b.tools[u], si, bool(u % 2))
        nswb = len(E.table(si, eight)[0]) - 1
        for s in range(2):
            ch = chans if s == 0 else chans[::-1][:2]
            _cce(b.cce[u, s], si, eight, nswb, E._random_lens(rng), (u + s) % 2, [(c, _gains(rng)) for c in ch],
                 tag=1 + 8 * s, rng=rng)
    return b


SLOT_CASES = ([({k}, set()) for k in (0, 7, 15)] +
              [({0, 15}, set()), ({3, 9}, {4, 5}), ({6, 7}, {0, 15})] +
              [(set(range(16)) - {k}, after) for k, after in ((0, set()), (5, {5}), (15, {15}), (9, set()))] +
              [(set(range(16)), set()), (set(range(16)), set())] +
              [({1, 4}, {2, 3}), ({2, 13}, {0, 1, 14, 15})])


def _slots(rng, pkg):
    b = _Batch(pkg, 2 * len(SLOT_CASES), MAX_CCE)
    nan = np.full(120, np.nan, np.float32)
    for u in range(len(b.tools)):
        spectral, after = SLOT_CASES[u % len(SLOT_CASES)]
        _target(rng, b.tools[u], 4 + u % 5, u >= len(SLOT_CASES))
        for s in range(MAX_CCE):
            si, eight = (s + u) % E.NUM_SI, bool((s + u // 2) % 2)
            nswb = len(E.table(si, eight)[0]) - 1
            rec = b.cce[u, s]
            if s in spectral:
                chans = [(s + u) % 2] if s % 3 else [s % 2, 1 - s % 2]
                _cce(rec, si, eight, nswb - s % 3, E._random_lens(rng), (s + u) % 2, [(c, _gains(rng)) for c in chans],
                     tag=s, rng=rng)
            else:
                # not for the spectral tools: an AFTER_IMDCT element, or no element at all (a stale record)
                _cce(rec, si, eight, nswb, E._random_lens(rng), AFTER_IMDCT if s in after else (s + u) % 2,
                     [(l % 2, nan) for l in range(MAX_LINKS)], tag=s, rng=rng)
                rec["present"] = 1 if s in after else 0
                b.poison[u, s] = True
    return b


ORDER_UNITS = 12


def order_exponents(j):
    """gain exponent of contribution j: low ones (0 .. -4) and high ones (12 .. 20) in turn, so that neighbours
    differ by 2^12 .. 2^24"""
    return -(j % 5) if j % 2 == 0 else 12 + (3 * j) % 9


def _order(rng, pkg):
    b = _Batch(pkg, ORDER_UNITS, MAX_CCE)
    for u in range(ORDER_UNITS):
        _target(rng, b.tools[u], u % E.NUM_SI, bool(u % 2), tns=0)
        for c in range(2):                                        # nothing but the sums: no noise, no intensity
            bt = b.tools[u]["ch"][c]["band_type"]
            bt[bt >= E.NOISE_BT] = 1
        for s in range(MAX_CCE):
            si, eight = (u + 5) % E.NUM_SI, bool((u // 2) % 2)
            nswb = len(E.table(si, eight)[0]) - 1
            lens = [1] * 8 if u % 4 == 2 else E._random_lens(rng)
            point = (u % 3) if u % 3 < 2 else s % 2
            links = []
            for c in range(2):
                j = s if u % 3 < 2 else s // 2                    # position among the point's contributions to c
                sign = np.float32(-1.0 if (j + c) % 2 else 1.0)
                links.append((c, np.full(120, sign * np.float32(2.0) ** order_exponents(j + c), np.float32)))
            bt = np.zeros(128, np.uint8)
            bt[: len(lens if eight else [1]) * nswb] = 1
            _cce(b.cce[u, s], si, eight, nswb, lens, point, links, tag=s, band_type=bt)
    return b


ZERO_PATTERNS = ("all_zero", "none_zero", "first_only", "last_only", "alternating")


def _zero_bands(rng, pkg):
    cases = [(p, eight, si) for p in ZERO_PATTERNS for eight in (False, True) for si in (3, 11)]
    b = _Batch(pkg, len(cases), 2)
    for u, (pattern, eight, si) in enumerate(cases):
        _target(rng, b.tools[u], si, bool(u % 2))
        nswb = len(E.table(si, eight)[0]) - 1
        for s in range(2):
            lens = E._random_lens(rng)
            nb = (len(lens) if eight else 1) * nswb
            bt = np.zeros(128, np.uint8)
            if pattern == "none_zero":
                bt[:nb] = rng.integers(1, 12, nb)
            elif pattern == "first_only":
                bt[0] = 5
            elif pattern == "last_only":
                bt[nb - 1] = 5
            elif pattern == "alternating":
                bt[s:nb:2] = 7
            links = []
            for c in (s, 1 - s):
                g = _gains(rng)
                g[bt[:120] == 0] = np.nan                         # (everything past the last band as well)
                links.append((c, g))
            _cce(b.cce[u, s], si, eight, nswb, lens, s, links, tag=2 + s, band_type=bt)
    return b


def golden_lists():
    """every golden gain in lists of 120: sorted by value and taken from both ends in turn (-inf beside +inf), then
    sorted by magnitude and taken from both ends in turn (the smallest beside the largest)"""
    flat = GOLDEN.ravel()
    out = []
    for key in (flat, np.abs(flat)):
        by = flat[np.argsort(key, kind="stable")]
        turn = np.empty_like(by)
        turn[0::2] = by[: (len(by) + 1) // 2]
        turn[1::2] = by[::-1][: len(by) // 2]
        pad = (-len(turn)) % 120
        out.append(np.concatenate([turn, turn[:pad]]).reshape(-1, 120))
    return np.concatenate(out)


def _gain_values(rng, pkg):
    lists = golden_lists()
    assert len(lists) % 2 == 0
    b = _Batch(pkg, len(lists) // 2, 1)
    bt = np.zeros(128, np.uint8)
    bt[:120] = 3
    for u in range(len(b.tools)):
        _target(rng, b.tools[u], 6 + u % 7, bool(u % 2), tns=0)
        _cce(b.cce[u, 0], 6 + (u * 3) % 7, True, 15, [1] * 8, u % 2, [(0, lists[2 * u]), (1, lists[2 * u + 1])], tag=u % 16,
             band_type=bt)
    return b


def _around_tns(rng, pkg):
    cases = [(o, d, eight, cce_eight) for o in TNS_TEMPLATE_ORDERS for d in (0, 1) for eight in (False, True)
             for cce_eight in (False, True)]
    b = _Batch(pkg, len(cases), 2)
    for u, (order, direction, eight, cce_eight) in enumerate(cases):
        fr = b.tools[u]
        si = (3, 6, 9, 0)[u % 4]
        _target(rng, fr, si, eight, tns=0)
        fr["ms_present"] = 1
        fr["ms_mask"] = rng.random(128) < 0.5
        fr["ch"][0]["band_type"][2] = E.NOISE_BT                  # the generator runs for certain
        fr["ch"][1]["band_type"][1] = E.INTENSITY_BT
        fr["ch"][1]["band_type"][3] = E.INTENSITY_BT2
        for c in range(2):
            ch = fr["ch"][c]
            ch["tns"]["present"] = 1
            nswb = int(ch["ics"]["num_swb"])
            for w in range(8 if eight else 1):
                ch["tns"]["n_filt"][w] = 1
                E._set_filter(rng, ch["tns"], w, 0, nswb, order, direction ^ (w & c & 1))
        nswb = len(E.table(si, cce_eight)[0]) - 1
        for s in range(2):
            lens = E._random_lens(rng)
            bt = np.zeros(128, np.uint8)
            bt[: (len(lens) if cce_eight else 1) * nswb] = rng.integers(1, 12, (len(lens) if cce_eight else 1) * nswb)
            # tags in descending point order on half of the units: the slot order is not the point order
            point = s if u % 2 else 1 - s
            _cce(b.cce[u, s], si, cce_eight, nswb, lens, point, [(0, _gains(rng)), (1, _gains(rng))], tag=4 + s,
                 band_type=bt)
    return b


_MAKE = dict(tables=_tables, groupings=_groupings, links=_links, slots=_slots, order=_order, zero_bands=_zero_bands,
             gains=_gain_values, around_tns=_around_tns)
_UNITS = {}
_ORACLE = {}


def units(pkg, profile, channels=2):
    """dict(tools [n], coeffs [n][channels][1024], cce [n][n_cce], cce_coeffs [n][n_cce][1024], rng [n]) of a
    profile: made once, shared, read-only.  A mono run reads channel 0 of the same records."""
    if profile not in _UNITS:
        k = PROFILES.index(profile)
        b = _MAKE[profile](np.random.default_rng([SEED, k]), pkg)
        assert b.cce.shape[1] == N_CCE[profile]
        n = len(b.tools)
        draw = np.random.default_rng([SEED, 100 + k])
        coeffs = (draw.standard_normal((n, 2, 1024)) * LEVEL).astype(np.float32)
        cc = (draw.standard_normal((n, b.cce.shape[1], 1024)) * LEVEL).astype(np.float32)
        cc[b.poison] = np.nan
        rs = draw.integers(-2**31, 2**31, n).astype(np.int32)
        rs[0] = E.RNG_START
        u = dict(tools=np.ascontiguousarray(b.tools), cce=np.ascontiguousarray(b.cce), cce_coeffs=cc, rng=rs,
                 coeffs={2: coeffs, 1: np.ascontiguousarray(coeffs[:, :1])})
        for a in (u["tools"], u["cce"], cc, rs, coeffs, u["coeffs"][1]):
            a.setflags(write=False)
        _UNITS[profile] = u
    u = _UNITS[profile]
    return dict(u, coeffs=u["coeffs"][channels])


def run_forms(tools_ex, stages, channels, u, form):
    """(coefficients, generator words) of one call form through tools_ex(channels, stages, coeffs, tools, rng=, cce=,
    cce_coeffs=) -> (coeffs, rng, ...): the oracle's binding, or the restatement's"""
    pre, post, both = stages
    kw = dict(cce=u["cce"], cce_coeffs=u["cce_coeffs"])
    if form == "all":
        r = tools_ex(channels, both, u["coeffs"], u["tools"], rng=u["rng"], **kw)
        return r[0], r[1]
    if form == "pre_post":
        r = tools_ex(channels, pre, u["coeffs"], u["tools"], rng=u["rng"])
        return tools_ex(channels, post, r[0], u["tools"], **kw)[0], r[1]
    r = tools_ex(channels, post, u["coeffs"], u["tools"], rng=u["rng"], **kw)
    return r[0], r[1]


def oracle_run(pkg, oracle, profile, channels, form):
    """the oracle on a profile: (coeffs [n][channels][1024], rng [n]); made once per case, shared, read-only"""
    key = (profile, channels, form)
    if key not in _ORACLE:
        out = run_forms(oracle.spectral_tools_batch_ex, (oracle.TOOLS_PRE, oracle.TOOLS_POST, oracle.TOOLS_ALL),
                        channels, units(pkg, profile, channels), form)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


# ---------------------------------------------------------------------------
# what the records hold
# ---------------------------------------------------------------------------
def check_record(rec):
    """a present or stale slot is inside what the parser writes"""
    ics = rec["ics"]
    nw, ng, nswb, m = (int(ics[k]) for k in ("num_windows", "num_window_groups", "num_swb", "max_sfb"))
    off = [int(x) for x in ics["swb_offset"][: nswb + 1]]
    assert nw in (1, 8) and off[0] == 0 and off[-1] == (128 if nw == 8 else 1024)
    assert all(b > a for a, b in zip(off, off[1:])) and E._si_of(ics)
    assert sum(int(x) for x in ics["group_len"][:ng]) == nw and not ics["group_len"][ng:].any()
    assert m <= nswb and ng * m <= 120 and int(rec["n_links"]) <= MAX_LINKS
    assert all(int(rec["link"][l]["target_ch"]) in (0, 1) for l in range(MAX_LINKS))


def reach(cce, tools=None):
    """what a batch of coupling records [n][n_cce] holds, as sets (spectral = present and not AFTER_IMDCT):
    tables {(si, windows)}, max_sfb_edge {(si, windows, 0 | 1 | 'num_swb-1' | 'num_swb')}, groupings {(num_swb,
    bits)} with max_sfb = num_swb, last_index {largest gain index read}, link_patterns {target_ch of four links},
    n_links, slot_counts {spectral slots per unit}, gaps / after_between / both_points (units), gains {words read},
    other_window {(coupling windows, target windows)}"""
    r = dict(tables=set(), max_sfb_edge=set(), groupings=set(), last_index=set(), link_patterns=set(), n_links=set(),
             slot_counts=set(), gaps=0, after_between=0, both_points=0, gains=set(), other_window=set(),
             twice=0, channel1_only=0)
    for u in range(cce.shape[0]):
        live = []
        for s in range(cce.shape[1]):
            rec = cce[u, s]
            if rec["present"] or int(rec["ics"]["num_windows"]):       # (a parser's empty slot is all zero)
                check_record(rec)
            if not rec["present"] or int(rec["coupling_point"]) == AFTER_IMDCT:
                continue
            live.append(s)
            ics = rec["ics"]
            nw, ng, nswb, m = (int(ics[k]) for k in ("num_windows", "num_window_groups", "num_swb", "max_sfb"))
            for si in E._si_of(ics):
                r["tables"].add((si, nw))
                for name, v in ((0, 0), (1, 1), ("num_swb-1", nswb - 1), ("num_swb", nswb)):
                    if m == v:
                        r["max_sfb_edge"].add((si, nw, name))
            if nw == 8 and m == nswb:
                r["groupings"].add((nswb, E.grouping_bits([int(x) for x in ics["group_len"][:ng]])))
            nl = int(rec["n_links"])
            r["n_links"].add(nl)
            chans = tuple(int(rec["link"][l]["target_ch"]) for l in range(nl))
            if nl == 4:
                r["link_patterns"].add(chans)
            r["twice"] += len(set(chans)) < len(chans)
            r["channel1_only"] += nl > 0 and set(chans) == {1}
            read = np.flatnonzero(rec["band_type"][: ng * m])
            if nl and len(read):
                r["last_index"].add(int(read[-1]))
                for l in range(nl):
                    r["gains"] |= set(int(x) for x in rec["link"][l]["gain"][read].view(np.uint32))
            if tools is not None:
                r["other_window"] |= {(nw, int(tools[u]["ch"][c]["ics"]["num_windows"])) for c in set(chans)}
        r["slot_counts"].add(len(live))
        if live:
            between = [s for s in range(live[0], live[-1]) if s not in live]
            r["gaps"] += any(not cce[u, s]["present"] for s in between)
            r["after_between"] += any(cce[u, s]["present"] for s in between)
            r["both_points"] += len({int(cce[u, s]["coupling_point"]) for s in live}) == 2
    return r


def contributions(u, k, c, point):
    """the addends of unit k's channel c at one coupling point, in the oracle's order (slots upwards, then links):
    [1024] float32 each, zero where the element's band walk writes nothing.  The oracle's expression, gain * src
    rounded to float, on the coupling channel's own grid."""
    out = []
    for s in range(u["cce"].shape[1]):
        rec = u["cce"][k, s]
        if not rec["present"] or int(rec["coupling_point"]) != point:
            continue
        ics = rec["ics"]
        for l in range(int(rec["n_links"])):
            if int(rec["link"][l]["target_ch"]) != c:
                continue
            a = np.zeros(1024, np.float32)
            idx = base = 0
            for g in range(int(ics["num_window_groups"])):
                for i in range(int(ics["max_sfb"])):
                    if rec["band_type"][idx]:
                        for w in range(int(ics["group_len"][g])):
                            lo = base + 128 * w + int(ics["swb_offset"][i])
                            hi = base + 128 * w + int(ics["swb_offset"][i + 1])
                            a[lo:hi] = rec["link"][l]["gain"][idx] * u["cce_coeffs"][k, s, lo:hi]
                    idx += 1
                base += 128 * int(ics["group_len"][g])
            out.append(a)
    return out


def order_property(pkg):
    """the `order` profile is what it is for: on every unit, channel and coupling point, folding the contributions in
    the oracle's order differs on at least one line from the fold with ANY two of them swapped, and neighbouring
    contributions differ by 2^12 .. 2^24 in gain and alternate in sign.  Returns the number of swaps tried."""
    u = units(pkg, "order")
    swaps = 0
    for k in range(len(u["tools"])):
        assert not u["tools"][k]["ch"]["tns"]["present"].any()
        for c in range(2):
            start = u["coeffs"][k, c]
            for point in (BEFORE_TNS, BETWEEN):
                adds = contributions(u, k, c, point)
                if len(adds) < 2:
                    continue
                ratio = [np.median(np.abs(adds[j + 1][adds[j] != 0]) / np.abs(adds[j][adds[j] != 0]))
                         for j in range(len(adds) - 1)]
                assert all(2.0 ** 8 < max(x, 1 / x) < 2.0 ** 28 for x in ratio), (k, c, point)

                def fold(order):
                    acc = start.copy()
                    for j in order:
                        acc = acc + adds[j]
                    return acc
                straight = list(range(len(adds)))
                ref = fold(straight)
                for a in range(len(adds)):
                    for b in range(a + 1, len(adds)):
                        o = list(straight)
                        o[a], o[b] = o[b], o[a]
                        assert not np.array_equal(fold(o), ref), (k, c, point, a, b)
                        swaps += 1
                start = ref
    return swaps


# ---------------------------------------------------------------------------
# independent coupling (heaac_couple_after_imdct_batch)
# ---------------------------------------------------------------------------
S16_TOP = np.float32(385.0 + 32767.0 / 32768.0)       # the largest float that is not clipped, and the smallest: 384
S16_STEP = np.float32(1.0 / 32768.0)                  # one int16 step = one ulp of the biased floats


def couple_case(pkg, n, channels, on, calls=3, seed=0):
    """records of `calls` chained heaac_couple_after_imdct_batch calls on one target: (pcm [n][channels][1024],
    [(cce [n][1024], coupling [n])]).  Outputs carry the decoder's bias (385 +- 1 is int16 full scale).  `on` is the
    (channel 0, channel 1) pattern; an uncoupled channel's gain is NaN.  Frame 0 of call 0 couples with gain 1 a
    coupling channel that is 0.25 on lines 0 .. 5: there the target sits so that the sum lands one step inside, on
    and one step outside the upper (lines 0 - 2) and the lower (lines 3 - 5) int16 limit."""
    rng = np.random.default_rng([SEED, 300, n, channels, int(on[0]), int(on[1]), seed])
    pcm = (BIAS + rng.standard_normal((n, channels, 1024)) * 0.3).astype(np.float32)
    steps = []
    for k in range(calls):
        cce = (BIAS + rng.standard_normal((n, 1024)) * 0.3).astype(np.float32)
        cpl = np.zeros(n, pkg.COUPLING_DT)
        cpl["on"][:, 0], cpl["on"][:, 1] = on
        g = _gains(rng)[:n] if n <= 120 else np.resize(_gains(rng), n)
        cpl["gain"][:, 0], cpl["gain"][:, 1] = g, g[::-1]
        cpl["gain"][cpl["on"] == 0] = np.nan
        if k == 0:
            cce[0, :6] = BIAS + np.float32(0.25)
            for c in range(channels):
                if on[c]:
                    cpl["gain"][0, c] = 1.0
                j = np.array([-1, 0, 1], np.float32) * S16_STEP
                pcm[0, c, 0:3] = S16_TOP - np.float32(0.25) + j
                pcm[0, c, 3:6] = np.float32(384.0) - np.float32(0.25) + j
        steps.append((cce, cpl))
    return pcm, steps


def couple_golden(pkg):
    """every golden gain through independent coupling: 257 frames (one per step) x 2 channels (positive, negative)
    x 4 chained calls (gain_element_scale 0 .. 3, the +-inf of scale 3 last: no NaN arises)"""
    rng = np.random.default_rng([SEED, 301])
    pcm = (BIAS + rng.standard_normal((257, 2, 1024)) * 0.3).astype(np.float32)
    steps = []
    for k in range(4):
        cce = (BIAS + rng.standard_normal((257, 1024)) * 0.3).astype(np.float32)
        cce[cce == BIAS] = BIAS + np.float32(0.125)
        cpl = np.zeros(257, pkg.COUPLING_DT)
        cpl["on"] = 1
        cpl["gain"][:, 0], cpl["gain"][:, 1] = GOLDEN[k], GOLDEN[4 + k]
        steps.append((cce, cpl))
    return pcm, steps


# ---------------------------------------------------------------------------
# interleave (heaac_pcm_interleave_batch)
# ---------------------------------------------------------------------------
def c_path_values():
    """all 65 536 floats 385 + k / 32768, k = -32768 .. 32767, in k's order"""
    return (np.arange(-32768, 32768, dtype=np.int64) + 0x43c08000).astype(np.uint32).view(np.float32)


def _neighbours(v):
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))])


def interleave_edges(sse2):
    """the edges of a conversion.  C path (the biased floats): the next float beyond either end, far beyond, +-inf
    and NaN.  SSE2 path (plain sample values): every tie k + 0.5 for k = -6 .. 5, +-32767.5, +-32768, the floats
    next to each of them, +-inf and NaN."""
    if sse2:
        v = _neighbours(np.concatenate([np.arange(-6, 6) + 0.5, [32767.5, -32767.5, 32768.0, -32768.0]]))
        far = [2147483648.0, -2147483648.0, 2147483520.0, -2147483904.0, 1e30, -1e30, 0.0, -0.0]
    else:
        v = np.array([np.nextafter(S16_TOP, np.float32(np.inf)), np.nextafter(np.float32(384), np.float32(-np.inf))])
        far = [386.5, 383.0, 512.0, 256.0, 255.9, 1e30, -1e30, 0.0, -385.5, -384.0, -1e30]
    return np.concatenate([v, np.array(far + [np.inf, -np.inf, np.nan], np.float32)]).astype(np.float32)


def interleave_pool(sse2, size):
    """`size` floats for the planes to point into: the conversion's edges (twice: a plane that starts a few floats
    in still reads them all), then every C-path float (or, for SSE2, samples around full scale), repeated"""
    size = max(size, 4)
    rng = np.random.default_rng([SEED, 400 + int(sse2)])
    if sse2:
        body = np.concatenate([interleave_edges(True)] * 2 + [(rng.standard_normal(4000) * 20000).astype(np.float32)])
    else:
        body = np.concatenate([interleave_edges(False)] * 2 + [c_path_values()[rng.permutation(65536)]])
    return np.resize(body, size).astype(np.float32)


def interleave_planes(channels, length, n):
    """([(offset, frame stride)] in floats, one per output channel; the floats the pool must hold): pairs in
    [n][2][len] buffers, single planes at a stride wider than len, one plane named by two output channels, one with
    frame_stride 0; bases and strides multiples of 4 floats"""
    planes, at, c = [], 0, 0
    while c < channels:
        kind = (c + channels) % 4
        if kind == 0 and c + 1 < channels:                         # a pair buffer
            planes += [(at, 2 * length), (at + length, 2 * length)]
            at += 2 * length * n
            c += 2
            continue
        if kind == 1:                                              # wider than len
            planes.append((at + 4, length + 8))
            at += 4 + (length + 8) * n
        elif kind == 2 and planes:                                 # the plane in front once more
            planes.append(planes[-1])
        elif kind == 3:                                            # every frame reads the same plane
            planes.append((at, 0))
            at += length
        else:
            planes.append((at, length))
            at += length * n
        c += 1
    assert all(o % 4 == 0 and s % 4 == 0 and o + (n - 1) * s + length <= at for o, s in planes)
    return planes, at
