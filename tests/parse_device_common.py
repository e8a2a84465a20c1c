"""Corpora and the comparison shared by test_parse_core.py (the walk on the host) and test_parse_device_gpu.py (the
same walk, one lane per unit): access units from the bit writer, the host parser heaac_aac_parse_frame_ex as the
reference, record bytes compared with numpy.  Nothing here knows how the walk under test is written."""
import contextlib
import ctypes as C

import numpy as np

import aac_bitwriter as W
import refused_units as RU
import test_parse as TP
import test_parse_wide as TW

FILL = 0xA5                      # every output byte before a call: float32 0xa5a5a5a5 is no value a parser writes


@contextlib.contextmanager
def no_pulses():
    """The bit writer's channels without pulse data (random_ics draws the same numbers either way)."""
    orig = W.random_ics

    def drawn(*a, **k):
        d = orig(*a, **k)
        d["pulse"] = None
        return d
    W.random_ics = drawn
    try:
        yield
    finally:
        W.random_ics = orig


def adts_header(aot, si, chan_config, payload_len, crc=False, blocks=0):
    bw = W.BitWriter()
    size = (9 if crc else 7) + payload_len
    for v, n in ((0xfff, 12), (0, 1), (0, 2), (0 if crc else 1, 1), (aot - 1, 2), (si, 4), (0, 1), (chan_config, 3), (0, 4),
                 (size & 0x1fff, 13), (0x7ff, 11), (blocks, 2)):
        bw.put(v, n)
    if crc:
        bw.put(0x1234, 16)
    return bw.bytes(pad=0)


def in_scope_steps(rng, si, aot, cpe, n, steps, adts=0.0, sbr=0.0):
    """steps x n access units the device walk must take: SCE / CPE without pulse data, DSE / FIL extras, some with an
    SBR payload behind the element, some behind an ADTS header (with and without a CRC)."""
    out = []
    with no_pulses():
        for _ in range(steps):
            row = []
            for _ in range(n):
                payload = None
                if rng.random() < sbr:
                    payload = ([int(x) for x in rng.integers(0, 2, int(rng.integers(4, 200)))], bool(rng.integers(0, 2)))
                au, _ = TP._write_au(rng, si, aot, cpe, extras=True, sbr=payload)
                if rng.random() < adts:
                    au = adts_header(aot, si, 2 if cpe else 1, len(au), crc=bool(rng.integers(0, 2))) + au
                row.append(au)
            out.append(row)
    return out


def main_high_order_units(rng, si, n):
    """AAC-Main SCE units on a long window whose one TNS filter has order 13 .. 20 (the bit writer stops at 12; AAC-LC
    refuses more): the max_order 20 branch and the last coefficients of HeaacTns.coef[..][..][20]."""
    out = []
    with no_pulses():
        while len(out) < n:
            d = W.random_ics(rng, si, 1, allow_intensity=False)
            if d["eight"]:
                continue
            order = 13 + len(out) % 8
            res, compress = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            d["tns"] = dict(n_filt=[1], coef_res=[res], filt=[[dict(
                length=int(rng.integers(0, d["num_swb"] + 1)), order=order, direction=int(rng.integers(0, 2)),
                compress=compress, idx=[int(x) for x in rng.integers(0, 1 << (res + 3 - compress), order)])]])
            bw = W.BitWriter()
            bw.put(0, 3); bw.put(0, 4)
            W.put_ics(bw, d, si, 1, 0)
            bw.put(7, 3)
            out.append((bw.bytes(), order))
    return out


def deferred_units(rng, si, aot, cpe, n):
    """Units the walk hands to the host: pulse data, coupling / program config elements, an LFE, two SCEs."""
    units = []
    while len(units) < n:                                      # pulse data in some channel
        au, e = TP._write_au(rng, si, aot, cpe, extras=True)
        if any(d["pulse"] for d in e["ch"]):
            units.append(au)
    with no_pulses():
        for i in range(n):                                     # test_parse_wide's coupling and program config units
            cces = [(int(t), [(1 if cpe else 0, 0, int(rng.integers(0, 4)) if cpe else 2)], int(rng.choice([0, 1, 3])),
                     bool(rng.integers(0, 2))) for t in rng.choice(16, int(rng.integers(0, 3)), replace=False)]
            units.append(TW.build_au(rng, si, aot, cpe, cces, pce=not cces or i % 3 == 0)[0])
        for _ in range(max(2, n // 4)):
            first = (RU.cpe_element if cpe else RU.sce_element)(rng, si, aot, "good")[0]
            lfe = RU.sce_element(rng, si, aot, "good", tag=0, lfe=True)[0]
            units.append(RU._bytes(first + lfe + RU.END))     # an LFE behind the output element
            second = RU.sce_element(rng, si, aot, "good", tag=1)[0]
            units.append(RU._bytes(first + second + RU.END))  # a second SCE
    return units


def damaged_units(rng, good, flips=400, randoms=200):
    """Truncations at every byte, bit flips and random buffers (the damage test_parse_fuzz.py's harness makes, and
    refused_units.py's written refusals)."""
    out = []
    for au in good[:3]:
        out += [au[:k] for k in range(1, len(au))]
    for _ in range(flips):
        au = bytearray(good[int(rng.integers(0, len(good)))])
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(0, len(au) * 8))
            au[k >> 3] ^= 0x80 >> (k & 7)
        out.append(bytes(au))
    for _ in range(randoms):
        out.append(bytes(rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8)))
    for _ in range(randoms // 4):                              # random bytes behind an ADTS sync word
        out.append(b"\xff\xf1" + bytes(rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8)))
    return out


def written_refusals(rng, si, aot, cpe):
    kinds = RU.KINDS_CPE if cpe else RU.KINDS_SCE
    return [(RU.cpe_unit if cpe else RU.sce_unit)(rng, si, aot, k)[0] for k in kinds for _ in range(3)]


_SF_CODES = {(int(l), int(c)): k for k, (c, l) in enumerate(zip(W.T["aac_sf_code"], W.T["aac_sf_bits"]))}


def classify(au, si, aot):
    """Which deferred class a unit THE HOST PARSER TAKES belongs to, read from its bits here (ISO/IEC 14496-3 tables
    4.4 - 4.50 with the bit writer's tables; no code of either parser): "element" for a CCE / LFE / PCE in front of the
    output element, "pulse" for pulse data in the first channel of the SCE / CPE, None if neither -- what lies behind
    the first channel's pulse flag (the second channel, elements behind the pair) is not followed."""
    bits = np.unpackbits(np.frombuffer(bytes(au), np.uint8)).tolist() + [0] * 96
    end = len(bits) - 96
    pos = 0

    def get(n):
        nonlocal pos
        v = 0
        for b in bits[pos:pos + n]:
            v = 2 * v + b
        pos += n
        return v

    def ics_info():
        nonlocal pos
        get(1)
        ws = get(2)
        get(1)
        if ws == 2:
            max_sfb = get(4)
            return True, max_sfb, 1 + sum(1 - get(1) for _ in range(7))
        max_sfb = get(6)
        if get(1):                                         # predictor data (AAC-Main; the host parser took the unit)
            if get(1):
                get(5)
            pos += min(max_sfb, W.T["aac_pred_sfb_max"][si])
        return False, max_sfb, 1

    if get(12) == 0xfff:
        pos = 56 if bits[15] else 72
    else:
        pos = 0
    while pos + 7 <= end:
        elem, tag = get(3), get(4)
        if elem == 7:
            return None
        if elem in (2, 3, 5):
            return "element"
        if elem == 4:
            align, cnt = get(1), get(8)
            if cnt == 255:
                cnt += get(8)
            if align:
                pos = (pos + 7) & ~7
            pos += 8 * cnt
            continue
        if elem == 6:
            pos += 8 * (tag + get(8) - 1 if tag == 15 else tag)
            continue
        common = get(1) if elem == 1 else 0
        if common:
            info = ics_info()
            if get(2) == 1:
                pos += info[1] * info[2]
        get(8)
        if not common:
            info = ics_info()
        eight, max_sfb, ng = info
        nb = 3 if eight else 5
        types = []
        for _ in range(ng):
            k = 0
            while k < max_sfb and pos < end:
                bt = get(4)
                n = get(nb)
                run = n
                while n == (1 << nb) - 1 and pos < end:
                    n = get(nb)
                    run += n
                types += [bt] * run
                k += run
        noise_first = True
        for bt in types:
            if bt == 0:
                continue
            if bt == 13 and noise_first:
                noise_first = False
                get(9)
                continue
            code = 0
            for length in range(1, 20):
                code = 2 * code + get(1)
                if (length, code) in _SF_CODES:
                    break
        return "pulse" if get(1) else None
    return None


def filled(pkg, n, cc, FILL=FILL):
    """Output arrays of n units with every byte set to FILL."""
    out = dict(coeffs=np.zeros((n, cc, 1024), np.float32), ics=np.zeros((n, cc), pkg.ICS_DT),
               tools=np.zeros(n, pkg.TOOLS_FRAME_DT), info=np.zeros(n, pkg.AAC_INFO_DT))
    for a in out.values():
        a.view(np.uint8)[...] = FILL
    return out


def host_parse(pkg, cfg, st, aus, cc, fill=FILL):
    """heaac_aac_parse_frame_ex(cfg, &st[i], au, size, cc, ..., cce = NULL, &info) per unit into FILLed arrays.
    st is updated in place (also by what a refused unit leaves).  Returns the arrays plus status [n]."""
    n = len(aus)
    out = filled(pkg, n, cc, fill)
    out["status"] = np.zeros(n, np.int32)
    f = pkg.lib().heaac_aac_parse_frame_ex
    p = {k: out[k].ctypes.data for k in ("coeffs", "ics", "tools", "info")}
    sp = st.ctypes.data
    for i, au in enumerate(aus):
        au = bytes(au)
        out["status"][i] = f(C.byref(cfg), C.c_void_p(sp + i * st.itemsize), au, len(au), cc,
                             C.c_void_p(p["coeffs"] + i * cc * 4096), C.c_void_p(p["ics"] + i * cc * 4),
                             C.c_void_p(p["tools"] + i * pkg.TOOLS_FRAME_DT.itemsize), None,
                             C.c_void_p(p["info"] + i * pkg.AAC_INFO_DT.itemsize))
    return out


def rows(a, n):
    return np.ascontiguousarray(a).view(np.uint8).reshape(n, -1)


def compare(pkg, cfg, st_before, aus, cc, got, st_after, fill=FILL):
    """The contract of heaac_aac_parse_device for one call, against the host parser from the same state:
      status OK        => the host returns OK; state, coefficient rows, ics, tools, info byte-identical (the outputs of
                          both were FILLed, so a byte either side leaves unwritten shows as well)
      host not OK      => DEFERRED
      DEFERRED         => the state bytes are as they were
    got: dict(coeffs, ics, tools, info, status) as numpy arrays.  Returns (host status [n], ok mask [n])."""
    n = len(aus)
    st_host = st_before.copy()
    host = host_parse(pkg, cfg, st_host, aus, cc, fill)
    status = np.asarray(got["status"]).reshape(n)
    assert set(np.unique(status)) <= {pkg.PARSE_OK, pkg.PARSE_DEFERRED}, np.unique(status)
    ok = status == pkg.PARSE_OK
    bad_ok = ok & (host["status"] != 0)
    assert not bad_ok.any(), ("OK on the device, refused by the host", np.flatnonzero(bad_ok)[:8], host["status"][bad_ok][:8])
    for k in ("coeffs", "ics", "tools", "info"):
        a, b = rows(got[k], n)[ok], rows(host[k], n)[ok]
        diff = (a != b).any(axis=1)
        assert not diff.any(), (k, np.flatnonzero(ok)[diff][:8], np.flatnonzero(a[diff][0] != b[diff][0])[:8])
    sa, sb, s0 = rows(st_after, n), rows(st_host, n), rows(st_before, n)
    assert np.array_equal(sa[ok], sb[ok]), ("state of OK units", np.flatnonzero(ok)[(sa[ok] != sb[ok]).any(axis=1)][:8])
    assert np.array_equal(sa[~ok], s0[~ok]), ("state of deferred units moved", np.flatnonzero(~ok)[(sa[~ok] != s0[~ok]).any(axis=1)][:8])
    return host["status"], ok
