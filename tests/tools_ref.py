"""The spectral tools once more, in numpy float32: an independent restatement that pins oracle/or_tools.c
(tests/test_tools_ref.py: bit identity on every profile of tests/edge_tools.py).  TEST INFRASTRUCTURE, CPU only: it is
not part of the product and no GPU test imports it.

Written from the reference's text -- decode_spectrum_and_dequant's NOISE_BT branch (aacdec.c:1003-1029), flt16_* /
predict / apply_prediction (:1247-1322), apply_mid_side_stereo and apply_intensity_stereo (:1390-1451), apply_tns
(:1698-1736) with compute_lpc_coefs (lpc.h:61-103) -- not from or_tools.c, and shaped the other way round: where the
reference walks groups, bands and windows, this maps every spectral LINE to its band (a search in the offsets) and
works on whole spectra; the noise generator is a table of composed steps; TNS runs all filters of a batch side by
side, serial in the line index only.  Every operation is one singly-rounded float32 operation in the reference's
order (the two variance sums of predict() in float64, as its double literal makes them), so the results are the
oracle's bit for bit.
"""
import numpy as np

F = np.float32
SF_SCALE = F(1.0 / (-1024.0 * 32768.0))        # ac->sf_scale on the C path (aacdec.c:575): negative
NOISE_BT, INTENSITY_BT2, INTENSITY_BT = 13, 14, 15
MAX_PREDICTORS = 672
LCG_A, LCG_C = np.uint32(1664525), np.uint32(1013904223)


def _lcg_tables(n):
    """x_j = A[j] x_0 + C[j] (mod 2^32), j = 0 .. n"""
    a = np.concatenate(([1], np.full(n, LCG_A))).astype(np.uint32)
    A = np.cumprod(a, dtype=np.uint32)
    C = np.concatenate(([0], np.cumsum(A[:-1], dtype=np.uint32) * LCG_C)).astype(np.uint32)
    return A, C


_A, _C = _lcg_tables(1024)


def line_bands(ics):
    """idx[1024]: the band index g * max_sfb + sfb of every spectral line of a channel, -1 above max_sfb"""
    nw, max_sfb, nswb = int(ics["num_windows"]), int(ics["max_sfb"]), int(ics["num_swb"])
    off = ics["swb_offset"][: nswb + 1].astype(np.int64)
    p = np.arange(1024)
    if nw == 8:
        group_of_window = np.repeat(np.arange(int(ics["num_window_groups"])),
                                    ics["group_len"][: int(ics["num_window_groups"])])
        g, k = group_of_window[p // 128], p % 128
    else:
        g, k = np.zeros(1024, np.int64), p
    sfb = np.searchsorted(off, k, side="right") - 1
    return np.where(sfb < max_sfb, g * max_sfb + sfb, -1)


def _pns(ch, coef, rs):
    """noise substitution on one channel: returns the generator word after it"""
    ics = ch["ics"]
    ng, max_sfb = int(ics["num_window_groups"]), int(ics["max_sfb"])
    nb = ng * max_sfb
    noise = np.flatnonzero(ch["band_type"][:nb] == NOISE_BT)
    if not len(noise):
        return rs
    off = ics["swb_offset"].astype(np.int64)
    lens = ics["group_len"][:ng].astype(np.int64)
    first_window = np.concatenate(([0], np.cumsum(lens)))[:ng]
    g, i = noise // max_sfb, noise % max_sfb
    # one row per (band, window of its group), in the order the generator runs through them
    reps = lens[g]
    band = np.repeat(np.arange(len(noise)), reps)
    window = np.repeat(first_window[g], reps) + (np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps))
    width = (off[i + 1] - off[i])[band]
    line0 = window * 128 + off[i][band]
    row_first = np.cumsum(width) - width                          # draws in front of the row
    total = int(width.sum())
    draws = (_A[1: total + 1] * np.uint32(rs & 0xffffffff) + _C[1: total + 1]).astype(np.uint32)
    value = draws.view(np.int32).astype(F)
    # rows side by side, the lines of a row left to right
    wmax = int(width.max())
    col = np.arange(wmax)
    live = col[None, :] < width[:, None]
    v = np.zeros((len(width), wmax), F)
    v[live] = value[(row_first[:, None] + col[None, :])[live]]
    energy = np.zeros(len(width), F)
    for k in range(wmax):
        energy = np.where(live[:, k], energy + v[:, k] * v[:, k], energy)
    scale = ch["sf"][noise][band] / np.sqrt(energy)
    out = v * scale[:, None]
    coef[(line0[:, None] + col[None, :])[live]] = out[live]
    return int(draws[-1].view(np.int32)) if total else rs


def _bits(x):
    return x.view(np.uint32)


def _even(x):
    b = _bits(x)
    return ((b + np.uint32(0x7fff) + (b & np.uint32(1))) & np.uint32(0xffff0000)).view(F)


def _round(x):
    return ((_bits(x) + np.uint32(0x8000)) & np.uint32(0xffff0000)).view(F)


def _trunc(x):
    return (_bits(np.ascontiguousarray(x, F)) & np.uint32(0xffff0000)).view(F)


def _prediction(ch, coef, st):
    """st [672][6] (cor0, cor1, var0, var1, r0, r1), in place"""
    ics, pr = ch["ics"], ch["pred"]
    if int(ics["num_windows"]) == 8:
        st[:] = (0, 0, 1, 1, 0, 0)
        return
    off = ics["swb_offset"].astype(np.int64)
    psm = int(pr["pred_sfb_max"])
    n = int(off[psm])
    k = np.arange(n)
    sfb = np.searchsorted(off[: psm + 1], k, side="right") - 1
    enable = (pr["prediction_used"][sfb] != 0) & bool(pr["predictor_present"])
    cor0, cor1, var0, var1, r0, r1 = (st[:n, j].copy() for j in range(6))
    a, alpha = F(0.953125), F(0.90625)
    k1 = np.where(var0 > 1, cor0 * _even(a / var0), F(0))
    k2 = np.where(var1 > 1, cor1 * _even(a / var1), F(0))
    pv = _round(k1 * r0 + k2 * r1)
    c = coef[:n]
    c = np.where(enable, c + pv * SF_SCALE, c)
    e0 = c / SF_SCALE
    e1 = e0 - k1 * r0
    st[:n, 1] = _trunc(alpha * cor1 + r1 * e1)
    st[:n, 3] = _trunc(((alpha * var1).astype(np.float64) + 0.5 * (r1 * r1 + e1 * e1).astype(np.float64)).astype(F))
    st[:n, 0] = _trunc(alpha * cor0 + r0 * e0)
    st[:n, 2] = _trunc(((alpha * var0).astype(np.float64) + 0.5 * (r0 * r0 + e0 * e0).astype(np.float64)).astype(F))
    st[:n, 5] = _trunc(a * (r0 - k1 * e0))
    st[:n, 4] = _trunc(a * e0)
    coef[:n] = c
    group = int(pr["predictor_reset_group"])
    if group:
        st[group - 1:: 30] = (0, 0, 1, 1, 0, 0)


def _mid_side(fr, c0, c1):
    idx = line_bands(fr["ch"][0]["ics"])
    safe = np.maximum(idx, 0)
    on = (idx >= 0) & (fr["ms_mask"][safe] != 0) & (fr["ch"][0]["band_type"][safe] < NOISE_BT) & \
        (fr["ch"][1]["band_type"][safe] < NOISE_BT)
    x, y = c0[on], c1[on]
    c0[on] = x + y
    c1[on] = x - y


def _intensity(fr, c0, c1):
    ch1 = fr["ch"][1]
    idx = line_bands(ch1["ics"])
    safe = np.maximum(idx, 0)
    bt = ch1["band_type"][safe].astype(np.int64)
    on = (idx >= 0) & ((bt == INTENSITY_BT) | (bt == INTENSITY_BT2))
    sign = -1 + 2 * (bt - 14)
    if fr["ms_present"]:
        sign = sign * (1 - 2 * fr["ms_mask"][safe].astype(np.int64))
    scale = sign.astype(F) * ch1["sf"][safe]
    c1[on] = scale[on] * c0[on]


def _tns(coeffs, tools, channels):
    """every filter of the batch at once: coeffs [n][channels][1024] in place"""
    base, start, inc, size, order, refl = [], [], [], [], [], []
    for f in range(len(tools)):
        for c in range(channels):
            ch = tools[f]["ch"][c]
            tns, ics = ch["tns"], ch["ics"]
            if not tns["present"]:
                continue
            mmm = min(int(ics["tns_max_bands"]), int(ics["max_sfb"]))
            off = ics["swb_offset"]
            for w in range(int(ics["num_windows"])):
                bottom = int(ics["num_swb"])
                for q in range(int(tns["n_filt"][w])):
                    top = bottom
                    bottom = max(0, top - int(tns["length"][w][q]))
                    o = int(tns["order"][w][q])
                    lo, hi = int(off[min(bottom, mmm)]), int(off[min(top, mmm)])
                    if o == 0 or hi <= lo:
                        continue
                    down = bool(tns["direction"][w][q])
                    base.append((f * channels + c) * 1024 + w * 128)
                    start.append(hi - 1 if down else lo)
                    inc.append(-1 if down else 1)
                    size.append(hi - lo)
                    order.append(o)
                    refl.append(tns["coef"][w][q])
    if not base:
        return
    # the longest filters first: the live ones are a prefix that shrinks as m grows
    by = np.argsort(-np.array(size), kind="stable")
    first = (np.array(base) + np.array(start))[by]
    inc, size, order = np.array(inc)[by], np.array(size)[by], np.array(order)[by]
    refl = np.array(refl, F)[by]
    nf = len(by)
    # compute_lpc_coefs: reflection coefficients to the predictor, filters side by side
    lpc = np.zeros((nf, 20), F)
    for i in range(int(order.max())):
        live = i < order
        r = -refl[:, i]
        new = lpc.copy()
        new[:, i] = r
        for j in range((i + 1) >> 1):
            f_, b_ = lpc[:, j], lpc[:, i - 1 - j]
            new[:, j] = f_ + r * b_
            new[:, i - 1 - j] = b_ + r * f_
        lpc[live] = new[live]
    flat = coeffs.reshape(-1)
    hist = np.zeros((nf, 20), F)                                  # the last outputs, newest first
    for m in range(int(size[0])):
        n = int(np.searchsorted(-size, -m, side="left"))          # filters with size > m
        pos = first[:n] + m * inc[:n]
        acc = flat[pos]
        lim = np.minimum(m, order[:n])
        for i in range(1, int(lim.max()) + 1):
            acc = np.where(i <= lim, acc - hist[:n, i - 1] * lpc[:n, i - 1], acc)
        flat[pos] = acc
        hist[:n, 1:] = hist[:n, :-1].copy()
        hist[:n, 0] = acc


def spectral_tools_batch(channels, coeffs, tools, rng=None, pred=None):
    """oracle_lib.spectral_tools_batch's signature and result"""
    out = np.ascontiguousarray(coeffs, F).copy()
    tools = np.ascontiguousarray(tools)
    n = out.shape[0]
    rout = None if rng is None else np.array(rng, np.int32)
    pout = None if pred is None else np.array(pred, F).reshape(n, channels, MAX_PREDICTORS, 6)
    with np.errstate(all="ignore"):
        for f in range(n):
            fr = tools[f]
            c0 = out[f, 0]
            c1 = out[f, 1] if channels == 2 else None
            if rout is not None:
                rs = int(rout[f])
                for c in range(channels):
                    rs = _pns(fr["ch"][c], out[f, c], rs)
                rout[f] = rs
            common = channels == 2 and bool(fr["common_window"])
            if pout is not None and not common:                   # decode_ics
                for c in range(channels):
                    _prediction(fr["ch"][c], out[f, c], pout[f, c])
            if channels == 2:
                if common and fr["ms_present"]:
                    _mid_side(fr, c0, c1)
                if pout is not None and common:                   # decode_cpe: behind M/S
                    for c in range(2):
                        _prediction(fr["ch"][c], out[f, c], pout[f, c])
                _intensity(fr, c0, c1)
        _tns(out, tools, channels)
    res = (out,) + ((rout,) if rng is not None else ()) + ((pout.reshape(np.shape(pred)),) if pred is not None else ())
    return res[0] if len(res) == 1 else res
