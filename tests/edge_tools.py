"""Structural profiles for the spectral tools (tests/test_tools_reach.py, tests/test_tools_ref.py,
tests/test_tools_grid_gpu.py).

Host logic only (numpy).  synth.tools_frames draws one band table (sampling index 3), TNS orders 0 .. 12 and 20, at
most 98 bands per channel and max_sfb >= 4; this module walks the rest of what a band table gives a HeaacToolsFrame:
every sampling index's long and short table with its tns_max_bands and pred_sfb_max, every TNS order in both
directions, all 128 groupings of eight short windows, 120-band channels full of noise, every predictor reset group.
The tables, tns_max_bands, pred_sfb_max and the TNS coefficient rows come from aac_bitwriter (the text of
csrc/aac_iso_tables.h); nothing is copied here.  The synth and its RNG draws are not touched; what this module draws
comes from generators of its own.

Every record stays inside what a band table gives: the offsets are a table's, group_len sums to 8 for eight short
windows, TNS coefficients are values of aac_tns_map (one row per filter: coef_res and coef_compress are per filter).
Orders up to 20 are used for long and short windows alike: the ABI takes them, the syntax caps a short window at 7.

A run is STREAMS x STEPS records [S][T] with spectra [S][T][channels][1024] in the synth's amplitude range
(+- 4096 SF_SCALE), state chained per stream from the decoder's start state.  The records do not depend on the
channel count: a mono run reads ch[0] of the same records.
"""
from collections import Counter

import numpy as np

import aac_bitwriter as W

PROFILES = ("tables", "tns_orders", "bands", "prediction")
STREAMS = 26
STEPS = 8
BANDS_STREAMS = 400                          # bands: 128 groupings x 3 short tables, one frame each, and the specials
BANDS_STEPS = 2
SEED = 20240611
SF_SCALE = 1.0 / (1024.0 * 32768.0)
NUM_SI = 13
NOISE_BT, INTENSITY_BT2, INTENSITY_BT = 13, 14, 15
RNG_START = 0x1f2e3d4c                       # ac->random_state at init (aacdec.c:567)

# (profile, the state the run carries) of the campaign: "pns_main" is the noise generator and the AAC-Main predictors,
# "none" neither (noise bands are taken as given); tables runs both ways, tns_orders needs no state
CASES = (("tables", "pns_main"), ("tables", "none"), ("tns_orders", "none"), ("bands", "pns_main"),
         ("prediction", "pns_main"))

# short tables by band count: sampling indices 0 - 2 have 12 bands, 3 - 5 have 14, 6 - 12 have 15
SHORT_CLASSES = {12: (0, 1, 2), 14: (3, 4, 5), 15: (6, 7, 8, 9, 10, 11, 12)}
TNS_LOW, TNS_MID = 7, 12                     # the order templates of k_tns / tools_tns_filter end here


def table(si, eight):
    """(swb offsets, tns_max_bands, pred_sfb_max) of sampling index si"""
    return (W.swb(si, eight), W.T["aac_tns_max_bands_128" if eight else "aac_tns_max_bands_1024"][si],
            W.T["aac_pred_sfb_max"][si])


def shape(profile):
    return (BANDS_STREAMS, BANDS_STEPS) if profile == "bands" else (STREAMS, STEPS)


def grouping_lens(bits):
    """group_len of scale_factor_grouping `bits` (7 bits, MSB first: 1 = window joins the group in front)"""
    lens, cur = [], 1
    for k in range(6, -1, -1):
        if (bits >> k) & 1:
            cur += 1
        else:
            lens.append(cur)
            cur = 1
    lens.append(cur)
    return lens


def grouping_bits(group_len):
    bits = 0
    for n in group_len:
        for k in range(int(n)):
            bits = (bits << 1) | (1 if k else 0)
    return bits & 0x7f


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------
def _set_ics(ics, si, eight, max_sfb, lens=None):
    off, tmb, _ = table(si, eight)
    assert 0 <= max_sfb <= len(off) - 1
    ics["num_windows"] = 8 if eight else 1
    ics["num_swb"] = len(off) - 1
    ics["tns_max_bands"] = tmb
    ics["max_sfb"] = max_sfb
    ics["swb_offset"][:] = 0
    ics["swb_offset"][: len(off)] = off
    lens = list(lens) if lens is not None else [1]
    assert sum(lens) == (8 if eight else 1)
    ics["num_window_groups"] = len(lens)
    ics["group_len"][:] = 0
    ics["group_len"][: len(lens)] = lens


def _random_lens(rng):
    return grouping_lens(int(rng.integers(0, 128)))


def _nb(ch):
    return int(ch["ics"]["num_window_groups"]) * int(ch["ics"]["max_sfb"])


def _mixed_bands(rng, ch, c):
    """band types and scalefactors in synth.tools_frames' shares: 10 % zero, 5 % noise, 20 % intensity on channel 1"""
    r = rng.random(128)
    bt = rng.integers(1, 12, 128)
    bt[r < 0.10] = 0
    bt[(r >= 0.10) & (r < 0.15)] = NOISE_BT
    if c == 1:
        bt[(r >= 0.15) & (r < 0.25)] = INTENSITY_BT2
        bt[(r >= 0.25) & (r < 0.35)] = INTENSITY_BT
    ch["band_type"] = bt
    ch["band_type"][_nb(ch):] = 0
    ch["sf"] = np.exp2(rng.integers(-12, 8, 128) / 4.0).astype(np.float32)


def _random_pred(rng, ch, si):
    pr = ch["pred"]
    pr["pred_sfb_max"] = table(si, False)[2]
    pr["predictor_present"] = rng.random() < 0.7
    pr["prediction_used"][:] = 0
    pr["prediction_used"][:41] = rng.random(41) < 0.6
    pr["predictor_reset_group"] = rng.integers(1, 31) if rng.random() < 0.15 else 0


def tns_coefs(rng, order):
    """20 reflection coefficients from one row of aac_tns_map, at every order alike.  All-pole filters of up to 20
    such sections grow large (tests/test_tools_reach.py asserts that they stay finite on these draws)."""
    row = np.array(W.T["tns_map"][int(rng.integers(0, 4))], np.float32)
    return row[rng.integers(0, len(row), 20)]


def _set_filter(rng, tns, w, k, length, order, direction):
    tns["length"][w][k] = length
    tns["order"][w][k] = order
    tns["direction"][w][k] = direction
    tns["coef"][w][k] = tns_coefs(rng, order)


def _random_tns(rng, ch, p_present=0.5):
    """as the synth draws it, with every order 0 .. 20 and coefficients of the table"""
    tns = ch["tns"]
    tns["present"] = rng.random() < p_present
    nw, nswb = int(ch["ics"]["num_windows"]), int(ch["ics"]["num_swb"])
    for w in range(nw):
        tns["n_filt"][w] = rng.integers(0, 2 if nw == 8 else 4)
        for k in range(int(tns["n_filt"][w])):
            _set_filter(rng, tns, w, k, int(rng.integers(0, nswb + 1)), int(rng.integers(0, 21)),
                        int(rng.integers(0, 2)))


def filter_ranges(ch):
    """[(window, filter, order, direction, bottom, top, start line, size)] of a channel as apply_tns lays the
    filters out (aacdec.c:1703-1720); size <= 0: the filter touches nothing"""
    ics, tns = ch["ics"], ch["tns"]
    out = []
    if not tns["present"]:
        return out
    mmm = min(int(ics["tns_max_bands"]), int(ics["max_sfb"]))
    off = ics["swb_offset"]
    for w in range(int(ics["num_windows"])):
        bottom = int(ics["num_swb"])
        for k in range(int(tns["n_filt"][w])):
            top = bottom
            bottom = max(0, top - int(tns["length"][w][k]))
            start, end = int(off[min(bottom, mmm)]), int(off[min(top, mmm)])
            out.append((w, k, int(tns["order"][w][k]), int(tns["direction"][w][k]), bottom, top, start, end - start))
    return out


def _spectra(rng, S, T):
    return ((rng.random((S, T, 2, 1024), dtype=np.float32) * 2 - 1) * np.float32(4096 * SF_SCALE)).astype(np.float32)


def _stereo(rng, fr, common):
    fr["common_window"] = common
    fr["ms_present"] = rng.integers(0, 3)
    fr["ms_mask"] = 1 if fr["ms_present"] == 2 else (rng.random(128) < 0.5)


# ---------------------------------------------------------------------------
# tables: all 13 sampling indices, long and short, max_sfb at every edge of the table
# ---------------------------------------------------------------------------
def max_sfb_choices(si, eight):
    off, tmb, psm = table(si, eight)
    nswb = len(off) - 1
    return [0, 1, tmb - 1, tmb] + ([tmb + 1] if tmb + 1 <= nswb else []) + ([psm] if psm <= nswb else []) + [nswb]


def _tables(rng, dt):
    S, T = shape("tables")
    t = np.zeros((S, T), dt)
    for s in range(S):
        si = s % NUM_SI
        for k in range(T):
            fr = t[s, k]
            # long and short alternate; the two streams of an index start on opposite sides and take the two halves
            # of the max_sfb cycle (at most 7 choices: every one comes up for long and for short)
            eight = bool((s // NUM_SI + k) % 2)
            turn = k // 2 + 4 * (s // NUM_SI)
            common = (s + k) % 3 != 0
            _stereo(rng, fr, common)
            ch0 = max_sfb_choices(si, eight)
            _set_ics(fr["ch"][0]["ics"], si, eight, ch0[turn % len(ch0)], _random_lens(rng) if eight else None)
            if common:
                fr["ch"][1]["ics"] = fr["ch"][0]["ics"]
            else:
                ch1 = max_sfb_choices(si, not eight)             # the other window length, another max_sfb
                _set_ics(fr["ch"][1]["ics"], si, not eight, ch1[(turn + 3) % len(ch1)],
                         None if eight else _random_lens(rng))
            for c in range(2):
                ch = fr["ch"][c]
                _mixed_bands(rng, ch, c)
                _random_pred(rng, ch, si)
                _random_tns(rng, ch)
    return t


# ---------------------------------------------------------------------------
# tns_orders
# ---------------------------------------------------------------------------
def order_class(s, k):
    """which orders frame k of stream s draws.  k_tns gives a (frame, channel) three lanes, so a wave holds 21 mono
    frames (10 stereo) adjacent in the call.  Streams 0 - 2 draw orders <= 7 throughout and streams 23 - 25 orders
    8 .. 12: 24 adjacent frames each in the streams form.  Position 6 of the other streams is <= 7 and position 7 is
    8 .. 12: 23 adjacent frames each in the batch form.  So each template is chosen by a whole wave in either form.
    Every other frame walks 0 .. 20, and its wave holds low, middle and high orders at once."""
    if s < 3:
        return "low"
    if s >= STREAMS - 3:
        return "mid"
    return "low" if k == 6 else "mid" if k == 7 else "mixed"


class _Walk:
    """(order, direction) in turn: every pair of 0 .. 20 x 2 once in 42 draws"""

    def __init__(self):
        self.n = 0

    def next(self):
        o, d = self.n % 21, (self.n // 21) % 2
        self.n += 1
        return o, d


def _long_lengths(pattern, nswb, mmm):
    """three filter lengths of a long window, by pattern; mmm = min(tns_max_bands, max_sfb) >= 6"""
    above = nswb - mmm
    third = mmm // 3
    if pattern == 0:                                             # tile num_swb exactly (the first one straddles mmm)
        return [above + third, third, mmm - 2 * third]
    if pattern == 1:                                             # overshoot: the bottom clamps to 0, the third is empty
        return [above + third, nswb, 5]
    if pattern == 2:                                             # a length of 0
        return [0, above + third, third]
    if pattern == 3:                                             # wholly above mmm (size 0), then the rest
        return [above, third, mmm - third]
    if pattern == 4:                                             # straddles mmm by two bands
        return [above + 2, 4, third]
    return [nswb - 1, 1, 0]                                      # 5: the second filter is the first band alone


def _tns_orders(rng, dt):
    S, T = shape("tns_orders")
    t = np.zeros((S, T), dt)
    walks = {(c, e): _Walk() for c in (0, 1) for e in (False, True)}
    for s in range(S):
        si = s % NUM_SI
        for k in range(T):
            fr = t[s, k]
            cls = order_class(s, k)
            eight = bool((s + k) % 2)
            pattern = (s * T + k) // 2 % 6
            _stereo(rng, fr, rng.random() < 0.7)
            for c in range(2):
                ch = fr["ch"][c]
                if c and fr["common_window"]:
                    ch["ics"] = fr["ch"][0]["ics"]
                else:
                    off, tmb, _ = table(si, eight)
                    nswb = len(off) - 1
                    max_sfb = nswb if (s + k + c) % 4 else tmb - 2     # mmm = tns_max_bands, or max_sfb below it
                    if eight and pattern == 5:
                        max_sfb = 1                                  # the one filter of a short window: one band
                    _set_ics(ch["ics"], si, eight, max_sfb, _random_lens(rng) if eight else None)
                ics, tns = ch["ics"], ch["tns"]
                _mixed_bands(rng, ch, c)
                _random_pred(rng, ch, si)
                nswb, mmm = int(ics["num_swb"]), min(int(ics["tns_max_bands"]), int(ics["max_sfb"]))
                short = int(ics["num_windows"]) == 8
                tns["present"] = 1
                walk = walks[c, short]
                for w in range(8 if short else 1):
                    if short:
                        # one filter per window: the whole window, overshooting, empty, above mmm, straddling it
                        lengths = [[nswb, nswb + 3, 0, nswb - mmm, nswb - mmm + 2][(w + s + k) % 5]]
                    else:
                        lengths = _long_lengths(pattern, nswb, mmm)
                    tns["n_filt"][w] = len(lengths)
                    for q, length in enumerate(lengths):
                        _set_filter(rng, tns, w, q, length, 0, 0)
                    for (_, q, _, _, bottom, top, start, size) in [f for f in filter_ranges(ch) if f[0] == w]:
                        one_band = pattern == 5 and size > 0 and min(top, mmm) == 1 and bottom == 0
                        if one_band and cls == "mixed":
                            order, direction = 20, int(rng.integers(0, 2))   # order > size: four lines
                        elif cls == "low":
                            order, direction = int(rng.integers(0, TNS_LOW + 1)), int(rng.integers(0, 2))
                        elif cls == "mid":
                            order, direction = int(rng.integers(TNS_LOW + 1, TNS_MID + 1)), int(rng.integers(0, 2))
                        elif size > 0:
                            order, direction = walk.next()           # the walk moves on filters that run
                        else:
                            order, direction = int(rng.integers(0, 21)), int(rng.integers(0, 2))
                        _set_filter(rng, tns, w, q, int(tns["length"][w][q]), order, direction)
    return t


# ---------------------------------------------------------------------------
# bands
# ---------------------------------------------------------------------------
SPECIALS = ("all_noise_120", "noise_64_119", "all_intensity", "ms_noise_one_side", "wide_and_narrow_noise",
            "max_sfb_0", "all_noise_long", "mixed_120")


def _special(rng, fr, kind, turn):
    si15 = SHORT_CLASSES[15][turn % 7]
    common = 1
    if kind in ("all_noise_120", "noise_64_119", "all_intensity", "ms_noise_one_side", "mixed_120"):
        _set_ics(fr["ch"][0]["ics"], si15, True, 15, [1] * 8)
        si = si15
    elif kind == "wide_and_narrow_noise":
        si = 3 + turn % 2
        _set_ics(fr["ch"][0]["ics"], si, False, 49)
    elif kind == "all_noise_long":
        si = turn % NUM_SI
        _set_ics(fr["ch"][0]["ics"], si, False, len(table(si, False)[0]) - 1)
    else:                                                        # max_sfb_0, long and short in turn
        si = turn % NUM_SI
        _set_ics(fr["ch"][0]["ics"], si, bool(turn % 2), 0, _random_lens(rng) if turn % 2 else None)
    _stereo(rng, fr, common)
    fr["ch"][1]["ics"] = fr["ch"][0]["ics"]
    for c in range(2):
        ch = fr["ch"][c]
        _mixed_bands(rng, ch, c)
        _random_pred(rng, ch, si)
        _random_tns(rng, ch, 0.3)
        nb = _nb(ch)
        bt = ch["band_type"]
        if kind in ("all_noise_120", "all_noise_long"):
            bt[:nb] = NOISE_BT
        elif kind == "noise_64_119":
            bt[:64] = rng.integers(1, 12, 64)
            bt[64:nb] = NOISE_BT
        elif kind == "all_intensity" and c == 1:
            bt[:nb] = np.where((np.arange(nb) + turn) % 2, INTENSITY_BT, INTENSITY_BT2)
        elif kind == "ms_noise_one_side":
            bt[:nb] = rng.integers(1, 12, nb)
            bt[c:nb:3] = NOISE_BT                                # idx = 0 mod 3 on channel 0, 1 mod 3 on channel 1
        elif kind == "wide_and_narrow_noise":
            bt[:nb] = rng.integers(1, 12, nb)
            bt[0] = bt[nb - 1] = NOISE_BT                        # 4 lines, 96 lines
    if kind == "all_intensity":
        fr["ms_present"] = turn % 3
        fr["ms_mask"] = 1 if fr["ms_present"] == 2 else (rng.random(128) < 0.5)
    elif kind == "ms_noise_one_side":
        fr["ms_present"] = 1 + turn % 2
        fr["ms_mask"] = 1


def _bands(rng, dt):
    S, T = shape("bands")
    t = np.zeros((S, T), dt)
    classes = sorted(SHORT_CLASSES)
    for s in range(S):
        for k in range(T):
            fr = t[s, k]
            if k == 0 and s < 384:
                # grouping s % 128 on the table class s // 128, the class's sampling indices in turn
                sis = SHORT_CLASSES[classes[s // 128]]
                si = sis[s % len(sis)]
                nswb = len(table(si, True)[0]) - 1
                _stereo(rng, fr, s % 4 != 0)
                _set_ics(fr["ch"][0]["ics"], si, True, nswb if s % 5 else nswb - 1, grouping_lens(s % 128))
                if fr["common_window"]:
                    fr["ch"][1]["ics"] = fr["ch"][0]["ics"]
                else:
                    _set_ics(fr["ch"][1]["ics"], si, True, nswb, grouping_lens((s * 37 + 11) % 128))
                for c in range(2):
                    ch = fr["ch"][c]
                    _mixed_bands(rng, ch, c)
                    _random_pred(rng, ch, si)
                    _random_tns(rng, ch, 0.3)
            else:
                _special(rng, fr, SPECIALS[(s + 4 * (1 - k)) % 8], s // 8)
    return t


# ---------------------------------------------------------------------------
# prediction (AAC-Main)
# ---------------------------------------------------------------------------
def _prediction(rng, dt):
    S, T = shape("prediction")
    t = np.zeros((S, T), dt)
    for s in range(S):
        si = s % NUM_SI
        off, _, psm = table(si, False)
        nswb = len(off) - 1
        for k in range(T):
            fr = t[s, k]
            eight = k == 3 or (k == 6 and s % 2 == 1)            # long -> short -> long: every predictor resets
            common = (s + k) % 2
            _stereo(rng, fr, common)
            fr["ms_present"] = 1 + k % 2                         # M/S on: its order against prediction matters
            fr["ms_mask"] = 1 if fr["ms_present"] == 2 else (rng.random(128) < 0.5)
            max_sfb = [psm - 5, psm, nswb][(s // NUM_SI + k) % 3]
            if eight:
                _set_ics(fr["ch"][0]["ics"], si, True, len(table(si, True)[0]) - 1, _random_lens(rng))
            else:
                _set_ics(fr["ch"][0]["ics"], si, False, max_sfb)
            if common:
                fr["ch"][1]["ics"] = fr["ch"][0]["ics"]
            elif (s + k) % 5 == 0 and not eight:                 # channel 1 alone goes short
                _set_ics(fr["ch"][1]["ics"], si, True, len(table(si, True)[0]) - 1, _random_lens(rng))
            else:
                fr["ch"][1]["ics"] = fr["ch"][0]["ics"]
                fr["ch"][1]["ics"]["max_sfb"] = [psm, nswb, psm - 5][(s // NUM_SI + k) % 3] if not eight else \
                    fr["ch"][0]["ics"]["max_sfb"]
            for c in range(2):
                ch = fr["ch"][c]
                _mixed_bands(rng, ch, c)
                _random_tns(rng, ch, 0.3)
                pr = ch["pred"]
                pr["pred_sfb_max"] = psm
                pr["predictor_present"] = (s + k + c) % 4 != 0   # a quarter: the state adapts, no output
                pr["prediction_used"][:] = 0
                pr["prediction_used"][:41] = rng.random(41) < 0.7
                pr["predictor_reset_group"] = (s * T + k + 7 * c) % 31
    return t


_MAKE = dict(tables=_tables, tns_orders=_tns_orders, bands=_bands, prediction=_prediction)


_FRAMES = {}
_CHAINS = {}


def frames(pkg, profile, channels=2):
    """(coeffs [S][T][channels][1024], tools [S][T]) of a profile: made once, shared, read-only"""
    if profile not in _FRAMES:
        rng = np.random.default_rng([SEED, PROFILES.index(profile)])
        tools = np.ascontiguousarray(_MAKE[profile](rng, pkg.TOOLS_FRAME_DT))
        S, T = tools.shape
        coeffs = _spectra(np.random.default_rng([SEED, 50 + PROFILES.index(profile)]), S, T)
        per = {2: coeffs, 1: np.ascontiguousarray(coeffs[:, :, :1])}
        for a in (tools, per[1], per[2]):
            a.setflags(write=False)
        _FRAMES[profile] = (per, tools)
    per, tools = _FRAMES[profile]
    return per[channels], tools


def oracle_chain(pkg, oracle, profile, channels, state):
    """the oracle frame position by frame position, the state chained: [(coeffs [S]..., rng [S], pred)] per position
    (None for a state the run does not carry); made once per case, shared, read-only"""
    key = (profile, channels, state)
    if key not in _CHAINS:
        coeffs, tools = frames(pkg, profile, channels)
        rs, pred = start_state(pkg, tools.shape[0], channels, state)
        out = []
        for t in range(tools.shape[1]):
            r = oracle.spectral_tools_batch(channels, coeffs[:, t], tools[:, t], rs, pred)
            r = list(r) if isinstance(r, tuple) else [r]
            c = r.pop(0)
            rs = r.pop(0) if rs is not None else None
            pred = r.pop(0) if pred is not None else None
            for a in (c, rs, pred):
                if a is not None:
                    a.setflags(write=False)
            out.append((c, rs, pred))
        _CHAINS[key] = out
    return _CHAINS[key]


def start_state(pkg, S, channels, state):
    """(generator words [S] or None, predictors [S][channels][672][6] or None): stream 0 from the decoder's start
    word, the others from words of their own; predictors from reset_all_predictors (aacdec.c:507-522)"""
    rs = pred = None
    if "pns" in state:
        rs = np.random.default_rng([SEED, 99]).integers(-2**31, 2**31, S).astype(np.int32)
        rs[0] = RNG_START
    if "main" in state:
        p = np.zeros((S, channels, pkg.MAX_PREDICTORS), pkg.PRED_STATE_DT)
        p["var0"] = 1.0
        p["var1"] = 1.0
        pred = np.ascontiguousarray(p.view(np.float32).reshape(S, channels, pkg.MAX_PREDICTORS, 6))
    return rs, pred


# ---------------------------------------------------------------------------
# what a run holds
# ---------------------------------------------------------------------------
def _si_of(ics):
    """the sampling indices whose table this is (several indices share a table)"""
    eight = int(ics["num_windows"]) == 8
    n = int(ics["num_swb"])
    return tuple(si for si in range(NUM_SI)
                 if list(ics["swb_offset"][: n + 1]) == list(W.swb(si, eight)) and
                 int(ics["tns_max_bands"]) == table(si, eight)[1])


def first_si(si, eight):
    """the lowest sampling index with the table and tns_max_bands of si (the key of max_sfb_at)"""
    return min(k for k in range(NUM_SI) if table(k, eight)[:2] == table(si, eight)[:2])


def tools_counts(tools, channels=2):
    """Counter over the records of a run ([S][T] or flat), channels 0 .. channels - 1"""
    c = Counter()
    for fr in np.asarray(tools).reshape(-1):
        c["frames"] += 1
        both_empty = True
        for k in range(channels):
            ch = fr["ch"][k]
            ics = ch["ics"]
            nw, nswb, max_sfb = int(ics["num_windows"]), int(ics["num_swb"]), int(ics["max_sfb"])
            ng = int(ics["num_window_groups"])
            lens = [int(x) for x in ics["group_len"][:ng]]
            off = [int(x) for x in ics["swb_offset"][: nswb + 1]]
            assert off[0] == 0 and off[-1] == (128 if nw == 8 else 1024) and all(b > a for a, b in zip(off, off[1:]))
            assert sum(lens) == nw and not ics["group_len"][ng:].any()
            for si in _si_of(ics):
                c["si", si, nw] += 1
            c["num_swb", nw, nswb] += 1
            c["max_sfb", max_sfb] += 1
            c["max_sfb_at", nw, _si_of(ics)[0], max_sfb] += 1
            if nw == 8:
                c["grouping", nswb, grouping_bits(lens)] += 1
            nb = ng * max_sfb
            both_empty = both_empty and nb == 0
            c["bands", nb] += 1
            bt = ch["band_type"][:nb]
            noise = np.flatnonzero(bt == NOISE_BT)
            c["noise_bands", len(noise)] += 1
            c["noise_second_round"] += int((noise >= 64).sum())
            c["second_round_full"] += nb == 120 and (noise >= 64).sum() == 56
            c["all_noise"] += nb > 0 and len(noise) == nb
            for idx in noise:
                i = idx % max_sfb
                c["noise_width", off[i + 1] - off[i]] += 1
            if k == 1:
                c["all_intensity", int(fr["ms_present"])] += nb > 0 and bool(np.isin(bt, (14, 15)).all())
            for (w, q, order, direction, bottom, top, start, size) in filter_ranges(ch):
                mmm = min(int(ics["tns_max_bands"]), max_sfb)
                if size > 0:
                    c["tns", nw, order, direction] += 1
                    c["order_gt_size"] += order > size
                    c["order20_on_4_lines"] += order == 20 and size == 4
                    c["straddle"] += top > mmm > bottom
                    c["clamped"] += int(ch["tns"]["length"][w][q]) > top > 0
                else:
                    c["empty_length_0"] += int(ch["tns"]["length"][w][q]) == 0
                    c["empty_above"] += bottom >= mmm and top > bottom
                    c["empty_after_clamp"] += top == 0
                c["tiles"] += q == int(ch["tns"]["n_filt"][w]) - 1 and bottom == 0 and \
                    sum(int(x) for x in ch["tns"]["length"][w][: q + 1]) == nswb
            pr = ch["pred"]
            if nw == 1:
                c["reset_group", int(pr["predictor_reset_group"])] += 1
                c["pred_sfb_max", int(pr["pred_sfb_max"])] += 1
                assert int(pr["pred_sfb_max"]) in {table(si, False)[2] for si in _si_of(ics)}
                c["adapt_no_output"] += (not pr["predictor_present"]) and bool(pr["prediction_used"].any())
                c["max_sfb_below_pred"] += max_sfb < int(pr["pred_sfb_max"])
                if channels == 2 and fr["ms_present"]:
                    c["pred_ms", int(fr["common_window"])] += 1
            else:
                c["pred_reset_all"] += 1
        if channels == 2:
            if fr["common_window"] and fr["ms_present"]:
                nb = _nb(fr["ch"][0])
                b0, b1 = fr["ch"][0]["band_type"][:nb], fr["ch"][1]["band_type"][:nb]
                m = fr["ms_mask"][:nb] != 0
                c["ms_skips_noise"] += int((m & ((b0 == NOISE_BT) != (b1 == NOISE_BT))).sum())
            c["windows_differ"] += int(fr["ch"][0]["ics"]["num_windows"]) != int(fr["ch"][1]["ics"]["num_windows"])
            c["max_sfb_differ"] += int(fr["ch"][0]["ics"]["max_sfb"]) != int(fr["ch"][1]["ics"]["max_sfb"])
        c["frame_max_sfb_0"] += both_empty
    return c


def keys(c, name):
    """the values counted under `name`: {rest of the key} of every (name, ...) entry above zero"""
    out = set()
    for k, v in c.items():
        if isinstance(k, tuple) and k[0] == name and v > 0:
            out.add(k[1] if len(k) == 2 else k[1:])
    return out


def tns_wave_classes(tools_flat, channels):
    """Counter of what the waves of k_tns hold over the frames of ONE call, in the call's order: a wave is 64 lanes,
    a (frame, channel) three of them, a lane's order counts when its filter runs (order > 0, size > 0).  Keys:
    "low" (every order <= 7, at least one filter), "mid" (the largest in 8 .. 12), "high", and "low+mid+high" for a
    wave that holds all three kinds at once."""
    lanes = []
    for fr in tools_flat:
        for k in range(channels):
            per = [0, 0, 0]
            for (w, q, order, _, _, _, _, size) in filter_ranges(fr["ch"][k]):
                if size > 0 and q < 3:
                    per[q] = max(per[q], order)                   # (windows are rounds of the same lane)
            lanes.extend(per)
    c = Counter()
    for first in range(0, len(lanes), 64):
        orders = [o for o in lanes[first: first + 64] if o > 0]
        if not orders:
            continue
        top = max(orders)
        c["low" if top <= TNS_LOW else "mid" if top <= TNS_MID else "high"] += 1
        c["low+mid+high"] += min(orders) <= TNS_LOW and top > TNS_MID and any(TNS_LOW < o <= TNS_MID for o in orders)
    return c
