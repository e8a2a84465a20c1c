"""Channel coupling once more, in numpy float32: an independent restatement that pins the coupling of
oracle/or_tools.c and oracle/or_core.c (tests/test_coupling_reach.py: bit identity on every profile of
tests/edge_coupling.py).  TEST INFRASTRUCTURE, CPU only: it is not part of the product and no GPU test imports it.

Written from the reference's text -- apply_dependent_coupling (aacdec.c:1813-1843), apply_independent_coupling
(:1849-1862), apply_channel_coupling (:1870-1898) and the two calls of spectral_to_sample (:1912, :1917) -- not from
or_tools.c, and shaped the other way round, as tests/tools_ref.py is: where the reference walks the coupling channel's
groups, bands and windows and adds into whatever lines they name, here every LINE of the target finds its window,
group and band in the coupling channel's grid (a search in its offsets), and a coupling element adds to all lines at
once.  The elements and their gain lists are an outer fold: tag order, then list order, which is the order the
reference's loops give a line's addends.  Each addend is gain * src rounded to float32, then one float32 add.

What this does NOT pin: that a coupling element's gain lists are resolved against the target as
apply_channel_coupling's index arithmetic resolves them (the parser does that, tests/test_parse_wide.py), and the
reference itself: its tree holds no vector for coupling, so this is the same reader twice.
"""
import numpy as np

import tools_ref as T

F = np.float32
BEFORE_TNS, BETWEEN_TNS_AND_IMDCT, AFTER_IMDCT = 0, 1, 3
PRE, POST = 1, 2
ADD_BIAS = F(385.0)


def line_grid(ics):
    """idx[1024]: for every spectral line the gain index g * max_sfb + sfb of the coupling channel's band that holds
    it, -1 where no band below max_sfb does"""
    p = np.arange(1024)
    nswb, max_sfb = int(ics["num_swb"]), int(ics["max_sfb"])
    off = ics["swb_offset"][: nswb + 1].astype(np.int64)
    if int(ics["num_windows"]) == 8:
        ng = int(ics["num_window_groups"])
        group_of_window = np.repeat(np.arange(ng), ics["group_len"][:ng])
        g, k = group_of_window[p >> 7], p & 127
    else:
        g, k = np.zeros(1024, np.int64), p
    sfb = np.searchsorted(off, k, side="right") - 1
    return np.where(sfb < max_sfb, g * max_sfb + sfb, -1)


def dependent_coupling(channels, coeffs, cce, cce_coeffs, point):
    """one coupling point on coeffs [n][channels][1024], in place"""
    for f in range(coeffs.shape[0]):
        for e in range(cce.shape[1]):                               # ac->che[TYPE_CCE][0 .. 15]
            rec = cce[f, e]
            if not rec["present"] or int(rec["coupling_point"]) != point:
                continue
            idx = line_grid(rec["ics"])
            safe = np.maximum(idx, 0)
            on = (idx >= 0) & (rec["band_type"][safe] != 0)
            src = cce_coeffs[f, e]
            for l in range(int(rec["n_links"])):
                c = int(rec["link"][l]["target_ch"])
                if c >= channels:
                    continue
                add = rec["link"][l]["gain"][safe[on]] * src[on]
                coeffs[f, c, on] = coeffs[f, c, on] + add


def spectral_tools_batch_ex(channels, stages, coeffs, tools, rng=None, pred=None, cce=None, cce_coeffs=None):
    """oracle_lib.spectral_tools_batch_ex's signature and result (no AAC-Main prediction here: pred must be None)"""
    assert pred is None
    out = np.ascontiguousarray(coeffs, F).copy()
    tools = np.ascontiguousarray(tools)
    rout = None if rng is None else np.array(rng, np.int32)
    with np.errstate(all="ignore"):
        if stages & PRE:
            for f in range(out.shape[0]):
                fr = tools[f]
                if rout is not None:
                    rs = int(rout[f])
                    for c in range(channels):
                        rs = T._pns(fr["ch"][c], out[f, c], rs)
                    rout[f] = rs
                if channels == 2:
                    if fr["common_window"] and fr["ms_present"]:
                        T._mid_side(fr, out[f, 0], out[f, 1])
                    T._intensity(fr, out[f, 0], out[f, 1])
        if stages & POST:
            if cce is not None:
                dependent_coupling(channels, out, cce, cce_coeffs, BEFORE_TNS)
            T._tns(out, tools, channels)
            if cce is not None:
                dependent_coupling(channels, out, cce, cce_coeffs, BETWEEN_TNS_AND_IMDCT)
    return out, rout, None


def s16_c(x):
    """float_to_int16_one (dsputil.c:3975-3980): the biased float's low 16 bits, clipped by what its high bits say"""
    t = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
    t = np.where(t & 0xf0000, -(((0x43c0ffff - t) & 0xffffffff) >> 31), t)       # (the subtraction wraps in 32 bits)
    return ((t - 0x8000) & 0xffff).astype(np.uint16).view(np.int16)


def s16_sse2(x):
    """cvtps2dq + packssdw (x86/dsputil_mmx.c:2356-2372): nearest even, NaN and |x| >= 2^31 are INT_MIN; clipped"""
    x = np.ascontiguousarray(x, F)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) < 2.0 ** 31, np.clip(np.rint(x.astype(np.float64)), -32768, 32767), -32768).astype(np.int16)


def couple_after_imdct_batch(channels, pcm, cce, coupling, s16=False):
    """oracle_lib.couple_after_imdct_batch's signature and result: every sample of a coupled channel at once"""
    out = np.ascontiguousarray(pcm, F).copy()
    cce = np.ascontiguousarray(cce, F)
    with np.errstate(all="ignore"):
        for c in range(channels):
            on = coupling["on"][:, c] != 0
            gain = coupling["gain"][on, c].astype(F)
            out[on, c] = out[on, c] + gain[:, None] * (cce[on] - ADD_BIAS)
    return out, (np.ascontiguousarray(s16_c(out).transpose(0, 2, 1)) if s16 else None)
