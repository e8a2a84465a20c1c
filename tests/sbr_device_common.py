"""Corpora and the comparison shared by test_sbr_core.py (the SBR / PS payload walk on the host) and
test_sbr_parse_device_gpu.py (the same walk, one lane per unit): HE-AAC access units from the two bit writers, the host
parser heaac_heaac_parse_frame_ex as the reference, record bytes compared with numpy.  Nothing here knows how the walk
under test is written."""
import contextlib
import copy
import ctypes as C

import numpy as np

import parse_device_common as PC
import sbr_bitwriter as SW
import test_parse as TP
import test_sbr_parse as TS

FILL = PC.FILL                   # every output byte before a call, on both sides: an unwritten byte shows up
SI, AOT = 6, 2                   # the core of test_sbr_parse._he_cfg: AAC-LC at 24 kHz under 48 kHz SBR
KX_AT, M_AT, HDR_AT = 16, 18, 20  # HeaacSbrStream: kx[2], m[2], hdr (include/heaac_parse.h)
STREAMS = [(False, "20"), (False, "34"), (False, "any"), (True, None)]      # (cpe, ps_modes): mono streams carry PS


def he_cfg(pkg, cpe):
    return TS._he_cfg(pkg, 2 if cpe else 1, not cpe)


def make_writers(pkg, n, cpe, ps_modes="any", ps=None):
    return [SW.SbrStreamWriter(pkg, 2 if cpe else 1, ps=(not cpe) if ps is None else ps, varfrac=0.6,
                               ps_modes=ps_modes or "any") for _ in range(n)]


def he_au(rng, cpe, payload=None, crc=False, misplaced=False):
    """One access unit: an SCE / CPE without pulse data (the device's AAC walk takes it), then a fill element with
    `payload` (the bits behind the 4-bit extension type) unless None; misplaced: a data stream element in between."""
    with PC.no_pulses():
        au, exp = TP._write_au(rng, SI, AOT, cpe, extras=False)
    bw = SW.Bits()
    bw.bits = np.unpackbits(np.frombuffer(au, np.uint8))[:exp["bits"] - 3].tolist()      # without the END element
    if misplaced:
        bw.put(4, 3); bw.put(0, 4); bw.put(0, 1); bw.put(1, 8); bw.put(0x55, 8)
    if payload is not None:
        cnt = (4 + len(payload) + 7) // 8
        assert cnt <= 269
        bw.put(6, 3)
        if cnt >= 15:
            bw.put(15, 4); bw.put(cnt - 14, 8)
        else:
            bw.put(cnt, 4)
        bw.put(0xe if crc else 0xd, 4)
        bw.bits.extend(int(x) for x in payload)
        bw.bits.extend([0] * (8 * cnt - 4 - len(payload)))
    bw.put(7, 3)
    return SW.to_bytes(bw.bits, pad=0)


def snapshot(w):
    """What a writer carries from frame to frame (restore() takes it back: a frame that was drawn but not sent)."""
    return copy.deepcopy((w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling))


def restore(w, snap):
    w.ch, w.ps, w.header, w.hdr_rec, w.kx_m, w.coupling = copy.deepcopy(snap)


def writer_frame(rng, w, new_header=False, respec=False, crc=False):
    """One payload of a writer that fits a single fill element (269 bytes)."""
    while True:
        keep = snapshot(w)
        bits, _ = w.frame(rng, new_header=new_header, crc=crc, respec=respec)
        if (4 + len(bits) + 7) // 8 <= 269:
            return bits
        restore(w, keep)


def he_units(rng, writers, cpe, new_header=False, respec=False, crc=False, before=None):
    aus = []
    for w in writers:
        if before:
            before(w)
        aus.append(he_au(rng, cpe, writer_frame(rng, w, new_header, respec, crc), crc))
    return aus


@contextlib.contextmanager
def resent_header(mode):
    """The header a writer re-sends on the same spectrum (frame(new_header=True)): "same" = the stream's header field
    for field, "limiter" = only bs_limiter_gains differs.  Yields a dict whose "header" entry the caller sets to the
    writer's current header ahead of each frame (draw_header draws the same numbers either way)."""
    orig = SW.draw_header
    state = {}

    def drawn(rng, spectrum=None):
        h = orig(rng, spectrum)
        if spectrum is None:
            return h
        h = dict(state["header"])
        if mode == "limiter":
            h["limiter_gains"] = (h["limiter_gains"] + 1) % 4
            h["extra_2"] = 1
        return h
    SW.draw_header = drawn
    try:
        yield state
    finally:
        SW.draw_header = orig


def filled(pkg, sst_like, n, with_ps, fill=FILL):
    """State-out and record arrays of n units with every byte set to `fill`."""
    out = dict(sst=np.zeros_like(sst_like[:n]), sbr=np.zeros(n, pkg.SBR_FRAME_DT), ps=np.zeros(n, pkg.PS_FRAME_DT) if with_ps else None)
    for a in out.values():
        if a is not None:
            a.view(np.uint8)[...] = fill
    return out


def host_parse(pkg, cfg, st, sst, tab, aus, cc, with_ps, fill=FILL):
    """heaac_heaac_parse_frame_ex per unit; st (AAC_STREAM_DT [n]) and sst (sbr_streams rows) are updated in place, the
    table takes the headers it meets.  Returns dict(status, sbr, ps, info); sbr / ps rows were `fill`ed."""
    n = len(aus)
    aac = PC.filled(pkg, n, cc, fill)
    out = filled(pkg, sst, n, with_ps, fill)
    out.pop("sst")
    out["info"] = aac["info"]
    out["status"] = np.zeros(n, np.int32)
    f = pkg.lib().heaac_heaac_parse_frame_ex
    at = lambda a, i, step: C.c_void_p(a.ctypes.data + i * step)
    for i, au in enumerate(aus):
        au = bytes(au)
        out["status"][i] = f(C.byref(cfg), at(st, i, st.itemsize), at(sst, i, sst.shape[1]), C.c_void_p(tab._h), au, len(au), cc,
                             at(aac["coeffs"], i, cc * 4096), at(aac["ics"], i, cc * pkg.ICS_DT.itemsize),
                             at(aac["tools"], i, pkg.TOOLS_FRAME_DT.itemsize), at(out["sbr"], i, pkg.SBR_FRAME_DT.itemsize),
                             at(out["ps"], i, pkg.PS_FRAME_DT.itemsize) if with_ps else None,
                             at(out["info"], i, pkg.AAC_INFO_DT.itemsize))
    return out


def compare(pkg, host, sst_host, sst_before, got):
    """The contract of heaac_sbr_parse_device for one call, against heaac_heaac_parse_frame_ex from the same state:
      status OK     => the host returns 0 or HEAAC_PARSE_NO_SBR; the state, sbr and ps rows are byte-identical (both
                       sides were FILLed)
      host anything else => DEFERRED
      DEFERRED      => the state-out row equals the state-in row
    host: what host_parse returned, sst_host: the states it left; got: dict(sst, sbr, ps, status).  Returns the ok mask."""
    n = len(host["status"])
    status = np.asarray(got["status"]).reshape(n)
    assert set(np.unique(status)) <= {pkg.PARSE_OK, pkg.PARSE_DEFERRED}, np.unique(status)
    ok = status == pkg.PARSE_OK
    host_takes = np.isin(host["status"], (0, pkg.PARSE_NO_SBR))
    bad = ok & ~host_takes
    assert not bad.any(), ("OK here, not on the host", np.flatnonzero(bad)[:8], host["status"][bad][:8])
    for k in ("sbr", "ps"):
        if host[k] is None:
            continue
        a, b = PC.rows(got[k], n)[ok], PC.rows(host[k], n)[ok]
        diff = (a != b).any(axis=1)
        assert not diff.any(), (k, np.flatnonzero(ok)[diff][:8], np.flatnonzero(a[diff][0] != b[diff][0])[:8])
    sa, sb, s0 = PC.rows(got["sst"], n), PC.rows(sst_host, n), PC.rows(sst_before, n)
    diff = (sa[ok] != sb[ok]).any(axis=1)
    assert not diff.any(), ("state of OK units", np.flatnonzero(ok)[diff][:8], np.flatnonzero(sa[ok][diff][0] != sb[ok][diff][0])[:8])
    moved = (sa[~ok] != s0[~ok]).any(axis=1)
    assert not moved.any(), ("state of deferred units moved", np.flatnonzero(~ok)[moved][:8])
    return ok


def aac_status_of(info):
    """The AAC half's status as the device reports it, from the host's info (channels = 0 where it refused the unit)."""
    return (info["channels"] == 0).astype(np.int32)


def payload_span(info):
    """(first bit, bits) of the unit's SBR payload from its info record."""
    return int(info["sbr_payload_bit"]), 8 * int(info["sbr_payload_bytes"]) - 4


def damaged(rng, aus, infos, flips=400, randoms=200, cpe=False):
    """(units, index of the stream each starts from): truncations at every byte of three units, `flips` units with
    1 - 3 bit flips inside the payload, `randoms` random payloads behind a good core."""
    units, src = [], []
    for i in range(3):
        units += [aus[i][:k] for k in range(1, len(aus[i]))]
        src += [i] * (len(aus[i]) - 1)
    for _ in range(flips):
        i = int(rng.integers(0, len(aus)))
        au = bytearray(aus[i])
        first, nbits = payload_span(infos[i])
        for _ in range(int(rng.integers(1, 4))):
            k = first + int(rng.integers(0, nbits))
            au[k >> 3] ^= 0x80 >> (k & 7)
        units.append(bytes(au))
        src.append(i)
    for au in PC.in_scope_steps(rng, SI, AOT, cpe, randoms, 1, sbr=1.0)[0]:
        units.append(au)
        src.append(int(rng.integers(0, len(aus))))
    return units, np.array(src)


CLASSES = ["plain", "plain", "plain", "same_header", "no_payload", "new_header", "limiter", "misplaced", "aac_refused",
           "bad_grid", "flipped", "truncated"]


def mixed_units(rng, writers, cpe, classes):
    """One unit per writer of the class named for it: the classes heaac_sbr_parse_device takes (a payload without a
    header, one that repeats the stream's header, no payload) and the ones it defers (a new spectrum, a limiter field,
    a misplaced payload, a unit the AAC half refuses, a malformed grid, damage).  A writer whose frame is damaged or
    withheld is set back, so that its next frame continues from what a decoder holds."""
    aus = []
    for w, cls in zip(writers, classes):
        keep = snapshot(w)
        crc = bool(rng.integers(0, 2))
        if cls in ("same_header", "limiter"):
            with resent_header("same" if cls == "same_header" else "limiter") as state:
                state["header"] = w.header
                au = he_au(rng, cpe, writer_frame(rng, w, new_header=True, crc=crc), crc)
        elif cls == "new_header":
            au = he_au(rng, cpe, writer_frame(rng, w, new_header=True, respec=True, crc=crc), crc)
        elif cls == "no_payload":
            au = he_au(rng, cpe)
        elif cls == "bad_grid":
            b = SW.Bits()
            b.put(0, 1); b.put(0, 1)
            if cpe:
                b.put(0, 1)
            for v, k in TS.BAD_GRIDS[int(rng.integers(0, len(TS.BAD_GRIDS)))]:
                b.put(v, k)
            au = he_au(rng, cpe, b.bits + [0] * 64)
        else:
            bits = writer_frame(rng, w, crc=crc)
            au = he_au(rng, cpe, bits, crc, misplaced=cls == "misplaced")
            if cls == "aac_refused":
                au = au[:3]
            elif cls == "truncated":
                au = au[:len(au) - 1 - int(rng.integers(0, max(1, len(bits) // 8 - 2)))]
            elif cls == "flipped":
                au = bytearray(au)
                for _ in range(int(rng.integers(1, 4))):
                    k = 8 * len(au) - 4 - int(rng.integers(0, len(bits)))
                    au[k >> 3] ^= 0x80 >> (k & 7)
                au = bytes(au)
        if cls in ("no_payload", "misplaced", "aac_refused", "bad_grid", "flipped", "truncated"):
            restore(w, keep)
        aus.append(au)
    return aus
