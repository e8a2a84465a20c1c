"""The parsers' structural campaign: corpora that reach every codeword of every code book the parsers walk (the AAC
scalefactor book and spectral books 1 - 11 with every book-11 escape length, the ten SBR books, the ten Parametric
Stereo books), the ends of every accumulator those codes feed (0 and 255 taken, one step outside refused), and the
section runs around the run-length escape.  Coverage comes from ENUMERATION: the writers (aac_bitwriter, sbr_bitwriter)
are driven by plans, an rng only fills in what does not matter (the AAC core under an HE payload).  The writers' own
models state what a parser must report; what was emitted is counted at the writers' emit functions (put_sf, put_spec,
Bits.huff) for as long as a corpus is being built (`counting`), so that the reach test holds exact sets against the
whole books.  test_codes_reach.py runs the corpora through the host parser and the walks on the host,
test_codes_gpu.py through the device parsers."""
import contextlib
import copy

import numpy as np

import aac_bitwriter as W
import sbr_bitwriter as SW
import sbr_device_common as SD

ERR_DATA = -1                                   # HEAAC_PARSE_ERR_DATA
BOOK_SIZE = {1: 81, 2: 81, 3: 81, 4: 81, 5: 81, 6: 81, 7: 64, 8: 64, 9: 169, 10: 169, 11: 289}
SIGN_PATTERNS = {3: 625, 4: 625, 7: 225, 8: 225, 9: 625, 10: 625, 11: 1089}      # sum over codewords of 2^(non-zero lines)


# ---- the counter ----
class Emitted:
    """What the writers' emit functions were asked for."""

    def __init__(self):
        self.sf = set()                         # scalefactor deltas
        self.spec = {b: set() for b in range(1, 12)}      # codeword indices per spectral book
        self.signed = {b: set() for b in SIGN_PATTERNS}   # (values) per unsigned book, escapes cut to +-16
        self.esc = set()                        # (prefix length N, value, negative, place in the pair)
        self.huff = {t: set() for t in SW.SBR_T + SW.PS_T}      # symbols per SBR / PS book

    def put_sf(self, delta):
        self.sf.add(int(delta))

    def put_spec(self, book, vals):
        if book <= 2:
            idx = sum((v + 1) * m for v, m in zip(vals, (27, 9, 3, 1)))
        elif book <= 4:
            idx = sum(abs(v) * m for v, m in zip(vals, (27, 9, 3, 1)))
        elif book <= 6:
            idx = (vals[0] + 4) * 9 + (vals[1] + 4)
        else:
            idx = min(abs(vals[0]), 16) * W.MOD[book] + min(abs(vals[1]), 16)
        self.spec[book].add(idx)
        if book in self.signed:
            self.signed[book].add(tuple(max(-16, min(16, int(v))) for v in vals))
        if book == 11:
            for place, v in enumerate(vals):
                if abs(v) >= 16:
                    self.esc.add((abs(v).bit_length() - 5, abs(v), v < 0, place, all(abs(x) >= 16 for x in vals)))


@contextlib.contextmanager
def counting(em=None):
    """The writers' emit functions report to `em` inside the block.  While the block runs the writers' MODULE GLOBALS
    (aac_bitwriter.put_sf, put_spec) and sbr_bitwriter.Bits.huff are rebound to counting wrappers -- whatever writes
    through the writers in that time is counted, the drawn corpora of the baseline test included -- and they are the
    writers' own again after it, also when the block raises (test_codes_reach.py asserts that)."""
    em = em or Emitted()
    put_sf, put_spec, huff = W.put_sf, W.put_spec, SW.Bits.huff

    def c_sf(bw, delta):
        em.put_sf(delta)
        put_sf(bw, delta)

    def c_spec(bw, book, vals):
        em.put_spec(book, vals)
        put_spec(bw, book, vals)

    def c_huff(self, table, sym):
        em.huff[table].add(int(sym))
        huff(self, table, sym)
    W.put_sf, W.put_spec, SW.Bits.huff = c_sf, c_spec, c_huff
    try:
        yield em
    finally:
        W.put_sf, W.put_spec, SW.Bits.huff = put_sf, put_spec, huff


# ---- a chain of differentially coded values ----
class Chain:
    """The deltas of one book still to be sent, for values that must stay in lo .. hi.  step(v) gives the next value:
    v plus the first pending delta that keeps it inside; if none does, a move (of at most `lav`) towards where the first
    pending one will; v itself once nothing is pending."""

    def __init__(self, lav, lo, hi, modulo=0):
        self.lav, self.lo, self.hi, self.modulo = lav, lo, hi, modulo
        order = [0]
        for d in range(lav, 0, -1):             # the longest codes first, the signs in turn: a zigzag
            order += [d, -d]
        self.pending = list(range(modulo)) if modulo else order

    def step(self, v):
        if self.modulo:
            return (v + (self.pending.pop(0) if self.pending else 0)) % self.modulo
        for k, d in enumerate(self.pending):
            if self.lo <= v + d <= self.hi:
                del self.pending[k]
                return v + d
        if not self.pending:
            return v
        d = self.pending[0]
        want = min(max(v, max(self.lo, self.lo - d)), min(self.hi, self.hi - d))
        return v + max(-self.lav, min(self.lav, want - v))


# =====================================================================================================================
# AAC
# =====================================================================================================================
def _unit(si, aot, chans, common=0, status=0, profile="", case=None):
    """One access unit from planned channels: an SCE, or a CPE (common: channel 1 shares channel 0's ics_info).
    Returns dict(au, exp = what test_parse._check_channel and its caller assert, status = what the host returns)."""
    bw = W.BitWriter()
    cpe = len(chans) == 2
    exp = dict(channels=len(chans), ch=chans, sbr_bit=-1)
    if cpe:
        bw.put(1, 3); bw.put(0, 4); bw.put(common, 1)
        exp.update(common_window=common, ms_present=0, ms_mask=np.zeros(128, np.uint8))
        if common:
            W.put_ics_info(bw, chans[0], si, aot)
            bw.put(0, 2)
    else:
        bw.put(0, 3); bw.put(0, 4)
    exp["sf"] = [W.put_ics(bw, d, si, aot, common) for d in chans]
    bw.put(7, 3)
    exp["bits"] = len(bw.bits)
    in_range = all(d["sf_in_range"] for d in chans)
    assert in_range == (status == 0) or case in ("escape_9", "run_past_max_sfb"), (profile, case)
    return dict(au=bw.bytes(), exp=exp, status=status, si=si, aot=aot, cpe=cpe, profile=profile, case=case)


GROUPINGS = [[1, 0, 1, 1, 0, 0, 1], [0, 1, 0, 1, 0, 1, 0], [0] * 7]      # 4, 5 and 8 groups of an eight-short frame
CHAIN_BT = dict(spectral=[1], noise=[13], intensity=[15, 14])


def _chain_channel(si, eight, chain, ch, start, k):
    """A channel whose every band is of `chain`'s kind, its deltas taken from ch (Chain) from the accumulator's start."""
    grouping = GROUPINGS[k % 2] if eight else None
    ms = len(W.swb(si, eight)) - 1
    ng = 1 + (7 - sum(grouping)) if eight else 1
    n = ng * ms
    types = [CHAIN_BT[chain][(j // 3) % len(CHAIN_BT[chain])] for j in range(n)]
    deltas, v = [], start
    for j in range(n):
        if chain == "noise" and j == 0:
            deltas.append(0)                    # the first noise band carries the 9-bit start
            continue
        nv = ch.step(v)
        deltas.append(nv - v)
        v = nv
    kw = dict(noise_level=start) if chain == "noise" else dict(global_gain=start if chain == "spectral" else 120)
    return W.planned_ics(si, eight, ms, types, deltas, grouping=grouping, **kw)


def sf_book(si=3, aot=2):
    """All 121 scalefactor deltas on each of the three chains, on a long window and on a grouped eight-short frame.
    Returns (units, tally): tally[(chain, eight)] = the deltas that chain was sent."""
    units, tally = [], {}
    k = 0
    for eight in (False, True):
        for chain in ("spectral", "noise", "intensity"):
            ch = Chain(60, 0, 255)
            seen = tally.setdefault((chain, eight), set())
            while ch.pending:
                d = _chain_channel(si, eight, chain, ch, 100 if chain == "intensity" else 128, k)      # positions start at 100
                if chain == "intensity":        # intensity positions belong to the second channel of a pair
                    first = W.planned_ics(si, eight, d["max_sfb"], [[1] * d["max_sfb"]] * len(d["group_len"]),
                                          grouping=d.get("grouping"))
                    units.append(_unit(si, aot, [first, d], common=k & 1, profile="sf_book"))
                elif k % 3 == 2:
                    other = _chain_channel(si, eight, "spectral", Chain(0, 0, 255), 100, k)
                    units.append(_unit(si, aot, [other, d], common=0, profile="sf_book"))
                else:
                    units.append(_unit(si, aot, [d], profile="sf_book"))
                first_noise = True
                for bt, dl in zip(d["band_type"].reshape(-1), d["sf_delta"].reshape(-1)):
                    if bt == 13 and first_noise:
                        first_noise = False
                        continue
                    seen.add(int(dl))
                k += 1
    return units, tally


def sf_ends(si=3, aot=2):
    """Each chain on 0 and on 255 (taken) and on -1 and 256 (HEAAC_PARSE_ERR_DATA), the 9-bit noise start at 0 and 511
    landing the noise accumulator on 0, on 255 and outside, global gain 0 and 255; each on a long window (sf_offset 0)
    and on an eight-short frame (sf_offset 12)."""
    units = []
    for eight in (False, True):
        ms = 6
        grouping = GROUPINGS[0] if eight else None
        ng = 4 if eight else 1

        def chan(bt, deltas, **kw):
            types = [[bt] * ms] * ng
            dl = np.zeros((ng, ms), int)
            dl.reshape(-1)[-len(deltas):] = deltas          # the landing is the last band of the last group
            return W.planned_ics(si, eight, ms, types, dl, grouping=grouping, **kw)

        def add(d, status, case, pair=False):
            if pair:
                first = W.planned_ics(si, eight, ms, [[2] * ms] * ng, grouping=grouping)
                units.append(_unit(si, aot, [first, d], common=int(eight), status=status, profile="sf_ends", case=case))
            else:
                units.append(_unit(si, aot, [d], status=status, profile="sf_ends", case=case))
        e = "short" if eight else "long"
        # spectral: global_gain + deltas
        add(chan(5, [-60, -60], global_gain=120), 0, ("spectral", 0, e))
        add(chan(5, [-60, -60, -1], global_gain=120), ERR_DATA, ("spectral", -1, e))
        add(chan(5, [55], global_gain=200), 0, ("spectral", 255, e))
        add(chan(5, [56], global_gain=200), ERR_DATA, ("spectral", 256, e))
        add(chan(5, [0], global_gain=0), 0, ("global_gain", 0, e))
        add(chan(5, [0], global_gain=255), 0, ("global_gain", 255, e))
        add(chan(5, [-1], global_gain=0), ERR_DATA, ("global_gain", -1, e))
        add(chan(5, [1], global_gain=255), ERR_DATA, ("global_gain", 256, e))
        # noise: the first band lands on noise_level, the deltas go on from there
        add(chan(13, [-60, -40], noise_level=100), 0, ("noise", 0, e))
        add(chan(13, [-60, -40, -1], noise_level=100), ERR_DATA, ("noise", -1, e))
        add(chan(13, [60, 35], noise_level=160), 0, ("noise", 255, e))
        add(chan(13, [60, 36], noise_level=160), ERR_DATA, ("noise", 256, e))
        # the 9 bits as sent: accumulator = global_gain - 90 + bits - 256
        add(chan(13, [0], global_gain=90, noise_start=511), 0, ("noise_start", 255, e))
        add(chan(13, [0], global_gain=91, noise_start=511), ERR_DATA, ("noise_start", 256, e))
        add(chan(13, [0], global_gain=255, noise_start=91), 0, ("noise_start", 0, e))
        add(chan(13, [0], global_gain=255, noise_start=90), ERR_DATA, ("noise_start", -1, e))
        add(chan(13, [0], global_gain=255, noise_start=0), ERR_DATA, ("noise_start", -91, e))
        # intensity positions: from 100
        add(chan(15, [-60, -40]), 0, ("intensity", 0, e), pair=True)
        add(chan(14, [-60, -40, -1]), ERR_DATA, ("intensity", -1, e), pair=True)
        add(chan(15, [60, 60, 35]), 0, ("intensity", 255, e), pair=True)
        add(chan(14, [60, 60, 36]), ERR_DATA, ("intensity", 256, e), pair=True)
    return units


def _spectral_items():
    """(book, values) for every codeword of books 1 - 11, the unsigned books with every sign pattern."""
    items = {}
    for book in range(1, 12):
        out = []
        dim = 4 if book <= 4 else 2
        lav = W.LAV[book] if book < 11 else 16
        mags = range(-lav, lav + 1) if book in (1, 2, 5, 6) else range(lav + 1)
        for idx in np.ndindex(*([len(mags)] * dim)):
            vals = [mags[i] for i in idx]
            if book in (1, 2, 5, 6):
                out.append(vals)
                continue
            nz = [i for i, v in enumerate(vals) if v]
            for s in range(1 << len(nz)):
                signed = list(vals)
                for bit, i in enumerate(nz):
                    if s >> bit & 1:
                        signed[i] = -signed[i]
                # 16 = the escape flag of book 11: an escaped value of its own (17 .. 31 by position, N = 0)
                out.append([int(np.sign(v)) * (17 + (len(out) % 15)) if abs(v) == 16 else v for v in signed])
        items[book] = out
    return items


def _fill_channels(si, items, ms):
    """Long-window channels whose bands take the items in order, one book per band; the last band of a book is padded
    with that book's first item."""
    off = W.swb(si, False)
    queue = [(book, v) for book in sorted(items) for v in items[book]]
    chans, pos = [], 0
    while pos < len(queue):
        types, q = [], {}
        for i in range(ms):
            if pos >= len(queue):
                types.append(0)
                continue
            book = queue[pos][0]
            step = 4 if book <= 4 else 2
            lines = []
            for _ in range((off[i + 1] - off[i]) // step):
                if pos < len(queue) and queue[pos][0] == book:
                    lines += queue[pos][1]
                    pos += 1
                else:
                    lines += items[book][0]
            types.append(book)
            q[(0, i)] = [lines]
        chans.append(W.planned_ics(si, False, ms, [types], q=q, global_gain=120))
    return chans


def _as_units(si, aot, chans, profile):
    """Channels as a mono unit, a pair without and a pair with a common window, in turn."""
    units, k = [], 0
    while chans:
        take = 1 if k % 3 == 0 or len(chans) == 1 else 2
        units.append(_unit(si, aot, chans[:take], common=int(k % 3 == 2), profile=profile))
        chans = chans[take:]
        k += 1
    return units


def spectral(si=3, aot=2):
    """Every codeword of spectral books 1 - 11 once (1 241), every sign pattern of the unsigned books."""
    return _as_units(si, aot, _fill_channels(si, _spectral_items(), len(W.swb(si, False)) - 1), "spectral")


def escapes(si=3, aot=2):
    """Every book-11 escape prefix length N = 0 .. 8 with its smallest and largest value, both signs, in either place of
    the pair and in both; N = 9 (refused)."""
    pairs = []
    for n in range(9):
        for v in (1 << (n + 4), (1 << (n + 5)) - 1):
            for s in (1, -1):
                pairs += [[s * v, 3], [-5, s * v], [s * v, -s * v], [s * v, 0], [0, s * v]]
    chans = _fill_channels(si, {11: pairs}, 40)
    units = _as_units(si, aot, chans, "escapes")                            # mono, and in either channel of a pair
    units += [_unit(si, aot, [copy.deepcopy(c), copy.deepcopy(c)], common=k, profile="escapes") for k, c in enumerate(chans * 2)]
    bad = W.planned_ics(si, False, 4, [[11] * 4], q={(0, 1): [[0, 0, 8192, 1]]}, global_gain=120)
    units.append(_unit(si, aot, [bad], status=ERR_DATA, profile="escapes", case="escape_9"))
    return units


def sections():
    """Section runs around the run-length escape (31 on a long window, 7 on a short one) and its multiples, a section
    that fills its group exactly, and one that runs a band past max_sfb (refused).  Long: the 51-band table (32 kHz),
    short: a 15-band table (24 kHz).  Returns units carrying case = the runs."""
    units = []
    si = 5
    ms = len(W.swb(si, False)) - 1
    assert ms == 51
    for first in (30, 31, 32, 51):
        types = [[1] * first + [3] * (ms - first)]
        units.append(_unit(si, 2, [W.planned_ics(si, False, ms, types)], profile="sections", case=("long", first)))
    units.append(_unit(si, 2, [W.planned_ics(si, False, ms, [[1] * ms], sections=[[(1, 20), (1, 31)]])], profile="sections",
                       case=("long", "equal_neighbours")))
    units.append(_unit(si, 2, [W.planned_ics(si, False, ms, [[1] * ms], sections=[[(1, ms + 1)]])], status=ERR_DATA,
                       profile="sections", case="run_past_max_sfb"))
    si = 6
    ms = len(W.swb(si, True)) - 1
    assert ms == 15
    runs = [6, 7, 8, 14, 15, 7, 14, 15]         # one per group of an ungrouped eight-short frame
    types = [[5] * r + [0] * (ms - r) for r in runs]
    units.append(_unit(si, 2, [W.planned_ics(si, True, ms, types, grouping=[0] * 7)], profile="sections", case=("short", tuple(runs))))
    units.append(_unit(si, 2, [W.planned_ics(si, True, ms, [[5] * ms] * 4, grouping=GROUPINGS[0],
                                             sections=[[(5, ms)], [(5, 7), (5, 8)], [(5, ms)], [(5, ms + 1)]])], status=ERR_DATA,
                       profile="sections", case="run_past_max_sfb"))
    return units


def aac_corpus():
    """Every AAC profile.  Returns (units, emitted, tally): units = dicts of _unit, tally of sf_book."""
    with counting() as em:
        book, tally = sf_book()
        units = book + sf_ends() + spectral() + escapes() + sections()
    return units, em, tally


_AAC = None


def aac_units():
    global _AAC
    if _AAC is None:
        _AAC = aac_corpus()
    return _AAC


def aac_groups(units):
    """{(si, aot, cpe): units}: what one configuration parses."""
    out = {}
    for u in units:
        out.setdefault((u["si"], u["aot"], u["cpe"]), []).append(u)
    return out


# =====================================================================================================================
# HE-AAC: SBR and Parametric Stereo
# =====================================================================================================================
def header(k, amp_res):
    return dict(SW.HEADERS[k], amp_res=amp_res, limiter_bands=2, limiter_gains=2, interpol_freq=1, smoothing_mode=1, extra_2=0)


class Books:
    """One Chain per SBR / PS book, made when a plan first asks for it."""

    def __init__(self):
        self.chains = {}
        self.classes = set()

    def chain(self, table, lo, hi, modulo=0):
        if table not in self.chains:
            lav = SW.T["sbr_lav"][table] if table in SW.SBR_T else SW.T["ps_offset"][table]
            self.chains[table] = Chain(lav, lo, hi, modulo)
        return self.chains[table]

    def pending(self, tables=None):
        return sum(len(c.pending) for t, c in self.chains.items() if tables is None or t in tables)


def _facs_plan(books, frame, what, constant=False):
    """The callable of Channel.put_envelope / put_noise: the direction whose book has more left to send, its values
    from the book's chain.  constant: a flat envelope in the frequency direction (a frame that is about something else)."""
    def plan(i, ref, nb, delta, tt, ft, start_bits):
        hi = 255 // delta
        if constant:
            return 0, [16 * delta] * nb
        ct, cf = books.chain(tt, 0, hi), books.chain(ft, 0, hi)
        if frame and len(ct.pending) >= len(cf.pending):
            books.classes.add((what, "time", frame["res_from"], frame["res"]) if what == "env" and i == 0 else (what, "time"))
            return 1, [delta * ct.step(r // delta) for r in ref]
        v = [min(16, (1 << start_bits) - 1)]
        while len(v) < nb:
            v.append(cf.step(v[-1]))
        books.classes.add((what, "freq"))
        return 0, [delta * x for x in v]
    return plan


def _he_frame(rng, w, cpe, plan, new_header=False, crc=False):
    """(au, exp) of a planned frame, or None where the payload does not fit one fill element (the writer is set back)."""
    keep = SD.snapshot(w)
    try:
        bits, exp = w.frame(None, new_header=new_header, crc=crc, plan=plan)
    except OverflowError:                       # an extension beyond its count field: longer than the element anyway
        bits = [0] * (8 * 270)
    if (4 + len(bits) + 7) // 8 > 269:
        SD.restore(w, keep)
        return None
    return SD.he_au(rng, cpe, bits, crc), exp


SBR_STREAMS = [(False, 0, 0, 0), (False, 0, 1, 3), (True, 0, 0, 0), (True, 0, 1, 3), (True, 1, 0, 0), (True, 1, 1, 3)]
RES = [0, 1, 1, 0]                              # bs_freq_res frame by frame: low->high, high->high, high->low, low->low


def sbr_books(pkg, rng, max_frames=60):
    """Chains of frames that send every codeword of the ten SBR books: mono, an uncoupled and a coupled pair, each with
    bs_amp_res 0 (the *_15 books) and 1 (the *_30 books), one of the two on a header with an odd high-resolution band
    count; the resolution changes between frames so that time deltas pass through both index mappings.
    Returns (streams, books): a stream = dict(cpe, with_ps, frames = [dict(au, exp, status, emitted = the symbols of this
    frame per book)], emitted = those of frames 1 .. only); frame 0 carries the header and a flat envelope, as the host
    parser alone reads it (the device registers no header)."""
    streams, all_books = [], []
    for cpe, coupling, amp_res, hk in SBR_STREAMS:
        books = Books()
        em = Emitted()
        w = SW.SbrStreamWriter(pkg, 2 if cpe else 1, ps=not cpe)
        frames = []
        h = header(hk, amp_res)
        while len(frames) < max_frames:
            k = len(frames)
            got = None
            for L in ((1,) if not k else (4, 2) if not cpe else (2,)):      # (FIXFIX with one envelope reads amp_res 0)
                res_from = w.ch[0].freq_res[w.ch[0].num_env]
                info = dict(res=RES[k % 4], res_from=res_from)
                keep = copy.deepcopy(books)
                chp = [dict(L=L, freq_res=RES[k % 4], env=_facs_plan(books, info, "env", not k),
                            noise=_facs_plan(books, info, "noise", not k)) for _ in range(2)]
                with counting() as tried:
                    got = _he_frame(rng, w, cpe, dict(header=h, coupling=coupling, ch=chp, ps=None), new_header=not k, crc=bool(k & 1))
                if got:
                    break
                books.chains, books.classes = keep.chains, keep.classes
            assert got, "a frame of one envelope must fit"
            frames.append(dict(au=got[0], exp=got[1], status=0, emitted=tried.huff))
            if k:                               # frame 0 carries the header: the device parsers are never handed it
                for t, syms in tried.huff.items():
                    em.huff[t] |= syms
            if k and not books.pending():
                break
        assert not books.pending(), ("codes left over", {t: c.pending for t, c in books.chains.items() if c.pending})
        streams.append(dict(cpe=cpe, with_ps=not cpe, frames=frames, kind=("sbr_books", cpe, coupling, amp_res), emitted=em,
                            classes=books.classes))
        all_books.append(books)
    return streams, all_books


PS_TABLES = {False: ("iid_df0", "iid_dt0"), True: ("iid_df1", "iid_dt1")}


def _ps_par(books, first):
    """The callable of PsModel._put_par: per envelope the direction whose book has more left, values from its chain.
    first: all zeros along frequency, no chain touched (frame 0 goes to the host parser only)."""
    def par(table_df, table_dt, e, prev, num):
        if first:
            return 0, [0] * num
        if table_df.startswith("iid"):
            lim = 15 if table_df.endswith("1") else 7
            lo, hi, modulo = -lim, lim, 0
        elif table_df.startswith("icc"):
            lo, hi, modulo = 0, 7, 0
        else:
            lo, hi, modulo = 0, 7, 8
        cd, ct = books.chain(table_df, lo, hi, modulo), books.chain(table_dt, lo, hi, modulo)
        if len(ct.pending) >= len(cd.pending):
            books.classes.add((table_dt, "frame border" if e == 0 else "envelope border"))
            return 1, [ct.step(p) for p in prev]
        out, v = [], 0
        for _ in range(num):
            v = cd.step(v)
            out.append(v)
        return 0, out
    return par


def ps_books(pkg, rng, max_frames=80):
    """Chains of mono frames that send every codeword of the ten Parametric Stereo books, once per band count: IID with
    10 / 20 / 34 bands in the coarse (modes 0 - 2) and the fine quantiser (3 - 5), ICC with 10 / 20 / 34, IPD / OPD with
    5 / 11 / 17; in the frequency direction and, across an envelope border and across a frame border, in the time
    direction.  The SBR part of each frame is a flat envelope; frame 0 (the SBR and the PS header) carries zeros, so that
    every codeword stands in a frame the device parsers are handed."""
    streams, all_books = [], []
    for mode in range(6):
        books = Books()
        em = Emitted()
        w = SW.SbrStreamWriter(pkg, 1, ps=True)
        frames = []
        flat = Books()
        while len(frames) < max_frames:
            k = len(frames)
            got = None
            for E in (4, 2, 1):
                keep = copy.deepcopy(books)
                ps = dict(header=(1, mode, 1, mode % 3, 1) if not k else None, num_env=E, ipdopd=1, par=_ps_par(books, not k))
                if k % 5 == 4:                  # transmitted borders; the last one short of the frame's end: one more envelope
                    ps.pop("num_env")
                    ps["borders"] = [7, 15, 23, 29][:E]
                chp = [dict(L=1, freq_res=0, env=_facs_plan(flat, None, "env", True), noise=_facs_plan(flat, None, "noise", True))]
                with counting() as tried:
                    got = _he_frame(rng, w, False, dict(header=header(0, 0), coupling=0, ch=chp, ps=ps), new_header=not k, crc=bool(k & 1))
                if got:
                    break
                books.chains, books.classes = keep.chains, keep.classes
            assert got, "a frame of one PS envelope must fit"
            frames.append(dict(au=got[0], exp=got[1], status=0, emitted=tried.huff))
            if k:                               # frame 0 carries the header: the device parsers are never handed it
                for t, syms in tried.huff.items():
                    em.huff[t] |= syms
            if k and not books.pending():
                break
        assert not books.pending(), ("codes left over", mode, {t: c.pending for t, c in books.chains.items() if c.pending})
        streams.append(dict(cpe=False, with_ps=True, frames=frames, kind=("ps_books", mode), emitted=em, classes=books.classes))
        all_books.append(books)
    return streams, all_books


def _ends_plan(values, what):
    """Channel plan whose envelope (what = "env") or noise floor (what = "noise") is `values` = (direction, [v] or v for
    every band, in units of the coding step), everything else flat."""
    def facs(i, ref, nb, delta, tt, ft, start_bits):
        df, v = values
        if df:                                  # the step once per frame: the envelopes behind the first repeat it
            return 1, [r + (delta * v if i == 0 else 0) for r in ref]
        v = list(v) + [v[-1]] * (nb - len(v))
        return 0, [delta * x for x in v[:nb]]
    flat = _facs_plan(Books(), None, "", True)
    return dict(L=2, freq_res=0, env=facs if what == "env" else flat, noise=facs if what == "noise" else flat)


def sbr_ends(pkg, rng):
    """Start values at 0 and at the top of their 7 / 6 / 6 / 5 / 5-bit fields, accumulated envelope and noise values on
    0 and on the top of the record's range (taken) and one coding step outside (refused: HEAAC_PARSE_ERR_DATA, the
    channel data rolled back -- the frame behind it, with a header, continues from the frame before).
    The field widths: 7 = envelope, bs_amp_res 0; 6 = envelope, bs_amp_res 1, and balance, bs_amp_res 0; 5 = balance,
    bs_amp_res 1, and every noise floor.  A balance channel moves in steps of 2: its top is 254, outside 256 and -2."""
    streams = []
    for cpe, coupling, amp_res, what, bits in ((False, 0, 0, "env", 7), (False, 0, 1, "env", 6), (True, 1, 0, "env", 6),
                                               (True, 1, 1, "env", 5), (False, 0, 0, "noise", 5), (True, 1, 1, "noise", 5)):
        bal = coupling == 1                                   # the case is about channel 1 of the coupled pair
        table = ("t_noise_bal_30" if bal else "t_noise_30") if what == "noise" else \
                ("t_env_bal_" if bal else "t_env_") + ("30" if amp_res else "15")
        lav, top = SW.T["sbr_lav"][table], (1 << bits) - 1
        hi = 127 if bal else 255
        for end in ("low", "high"):
            w = SW.SbrStreamWriter(pkg, 2 if cpe else 1, ps=not cpe)
            h = header(0, amp_res)
            frames = []

            def send(values, status=0, new_header=False):
                flat = _ends_plan((0, [16]), "")
                mine = _ends_plan(values, what)
                chp = [flat, mine] if bal else [mine, mine]
                keep = SD.snapshot(w)
                au, exp = _he_frame(rng, w, cpe, dict(header=h, coupling=coupling, ch=chp, ps=None), new_header=new_header)
                if status:
                    SD.restore(w, keep)
                frames.append(dict(au=au, exp=exp if not status else None, status=status, case=(what, bits, end, values), emitted={}))
            if end == "low":
                send((0, [0]), new_header=True)               # start value 0: lands on 0
                send((1, -1), status=ERR_DATA)                # one step below
            else:
                send((0, [top]), new_header=True)             # start value at the top of its field
                v = top
                while v < hi:
                    step = min(lav, hi - v)
                    send((1, step))
                    v += step                                 # ... lands on the top of the record's range
                send((1, 1), status=ERR_DATA)                 # one step above
            send((0, [16]), new_header=True)                  # the stream goes on from the frame before the refused one
            send((1, 1))
            streams.append(dict(cpe=cpe, with_ps=not cpe, frames=frames, kind=("sbr_ends", cpe, amp_res, what, bits, end),
                                emitted=Emitted(), classes=set()))
    return streams


def he_corpus(pkg):
    """Every HE profile.  Returns (streams, emitted): each stream also carries what it alone emitted (sbr_books,
    ps_books) and the classes its plans met; emitted = the union over the two book profiles."""
    rng = np.random.default_rng(4242)           # only the AAC core under each payload is drawn
    streams = sbr_books(pkg, rng)[0] + ps_books(pkg, rng)[0] + sbr_ends(pkg, rng)
    em = Emitted()
    for s in streams:
        for t, syms in s["emitted"].huff.items():
            em.huff[t] |= syms
    return streams, em


_HE = None


def he_streams(pkg):
    global _HE
    if _HE is None:
        _HE = he_corpus(pkg)
    return _HE


class HeItems:
    """The HE corpus behind the host parser: every frame of every stream of one channel configuration with the states the
    host parser held in front of it, so that any set of frames (or of runs of T frames) can share one call, each from
    its own state.  Frame 0 of a stream carries its header and is parsed here (the device registers none)."""

    def __init__(self, pkg, streams, cpe):
        self.pkg, self.cpe = pkg, cpe
        self.cfg = SD.he_cfg(pkg, cpe)
        self.with_ps, self.cc = not cpe, 2 if cpe else 1
        self.tab = pkg.SbrHeaderTable(256)
        self.streams = [s for s in streams if s["cpe"] == cpe]
        self.items = []                         # (stream, frame, AAC state before, SBR state before)
        self.host = []                          # per stream: dict(status, sbr, ps) of every frame
        for k, s in enumerate(self.streams):
            st = np.zeros(1, pkg.AAC_STREAM_DT)
            sst = pkg.sbr_streams(1)
            rec = []
            for t, f in enumerate(s["frames"]):
                before = (st.copy(), sst.copy())
                h = SD.host_parse(pkg, self.cfg, st, sst, self.tab, [f["au"]], self.cc, self.with_ps)
                rec.append(dict(status=int(h["status"][0]), sbr=h["sbr"], ps=h["ps"], st=before[0], sst=before[1], sst_after=sst.copy()))
                if t:
                    self.items.append((k, t))
            self.host.append(rec)

    def rows(self, picks, T):
        """rows[t][s], AAC states [S] and SBR states [S] for runs of T frames starting at the (stream, frame) picks
        (a run that reaches past its stream's end ends in empty units, which stop it)."""
        rows = [[(self.streams[k]["frames"][t + j]["au"] if t + j < len(self.streams[k]["frames"]) else b"") for k, t in picks]
                for j in range(T)]
        st = np.concatenate([self.host[k][t]["st"] for k, t in picks])
        sst = np.concatenate([self.host[k][t]["sst"] for k, t in picks])
        return rows, st, sst


def whole_books(tables):
    return {t: set(range(len(SW.T[t][0]))) for t in tables}


MONO_SBR_T = ["t_env_15", "f_env_15", "t_env_30", "f_env_30", "t_noise_30"]      # no balance books without a coupled pair


def books_of(cpe):
    """The books a channel configuration's frames reach whole: mono the unbalanced SBR books and all ten PS books, the
    pairs (coupled and not) all ten SBR books."""
    return whole_books(SW.SBR_T if cpe else MONO_SBR_T + SW.PS_T)


def symbols_handed(items, picks, taken):
    """{book: symbols} over the frames a call took: `taken[i]` frames from pick i = (stream, frame) of HeItems."""
    out = {t: set() for t in SW.SBR_T + SW.PS_T}
    for (k, t), n in zip(picks, taken):
        for f in items.streams[k]["frames"][t:t + int(n)]:
            for table, syms in f["emitted"].items():
                out[table] |= syms
    return out


def spread(n_items, n, seed):
    """n picks out of n_items: a fixed permutation, so that neighbours in a call come from different places of the corpus
    (the 1-bit codes next to the 20-bit ones, refused units next to taken ones), repeated if n is larger."""
    perm = np.random.default_rng(seed).permutation(n_items)
    return [int(perm[i % n_items]) for i in range(n)]


def run_walk(pkg, one, call, cfg, st, rows, cc, sst=None, hdr=None, with_ps=False, tab=None):
    """One streams call of T = len(rows) units per lane, each lane from its own state, held three ways: the one-unit
    forms (`one`: parse_streams_common.HostOne, or the device calls) position by position against the host parser
    (parse_device_common.compare, sbr_device_common.compare), the streams call (`call(cfg, st, rows, cc, sst, hdr,
    with_ps)` -> (outputs, AAC states after), every output pre-filled) byte for byte against that model, and the host
    parser's chain over the same units (parse_streams_common.check_against_host).  Returns the call's outputs."""
    import parse_streams_common as PS
    T, S = len(rows), len(rows[0])
    mdl = PS.model(pkg, one, cfg, st, rows, cc, sst, hdr, with_ps, tab, host_check=True)
    got, after = call(cfg, st, rows, cc, sst, hdr, with_ps)
    PS.compare_with_model(pkg, got, after, mdl, S, T)
    PS.check_against_host(pkg, cfg, got, after, st, rows, cc, sst, tab, with_ps)
    return got
