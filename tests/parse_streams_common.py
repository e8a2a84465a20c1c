"""What test_parse_streams_core.py (the chains of csrc/parse_streams.h on the host) and test_parse_streams_gpu.py (the
same chains, one lane per stream) share: the reference model of a streams call -- the ONE-UNIT forms run position by
position, stopped streams masked out, states put back where the SBR half alone gave a unit up -- the all-host chain
(heaac_aac_parse_frame_ex / heaac_heaac_parse_frame_ex unit by unit), and the comparisons.  Nothing here knows how the
chain under test is written.

Units are handed around as rows[t][s] (position-major, as the corpora of parse_device_common / sbr_device_common
come); a streams call takes them flat, unit t of stream s at s * T + t (`flat`)."""
import numpy as np

import parse_device_common as PC
import refused_units as RU
import sbr_device_common as SD
import test_parse as TP
import test_parse_wide as TW

AAC_KEYS = ("coeffs", "ics", "tools", "info")
HE_KEYS = AAC_KEYS + ("sbr", "ps")


def flat(rows):
    T, S = len(rows), len(rows[0])
    return [rows[t][s] for s in range(S) for t in range(T)]


def filled_streams(pkg, S, T, cc, sst_like=None, with_ps=False, fill=PC.FILL):
    """Every output of a streams call with each byte set to `fill`."""
    n = S * T
    out = PC.filled(pkg, n, cc, fill)
    out.update(status=np.zeros(n, np.int32), taken=np.zeros(S, np.uint32), hold=np.zeros(n, np.uint8), why=np.zeros(n, np.int32))
    if sst_like is not None:
        he = SD.filled(pkg, sst_like, n, with_ps, fill)
        out.update(sst=np.zeros_like(sst_like), sbr=he["sbr"], ps=he["ps"])
    for k in ("status", "taken", "hold", "why", "sst"):
        if k in out:
            out[k].view(np.uint8)[...] = fill
    return out


class HostOne:
    """The one-unit forms on the host: heaac_debug_aac_parse_core and heaac_debug_sbr_parse_core."""

    def __init__(self, pkg):
        self.pkg = pkg

    def aac(self, cfg, st, aus, cc):
        return self.pkg.aac_parse_core(cfg, st, aus, coeff_channels=cc, out=PC.filled(self.pkg, len(aus), cc))

    def sbr(self, cfg, sst, aus, info, hdr, status, with_ps):
        return self.pkg.sbr_parse_core(cfg, sst, aus, info, hdr, status, with_ps, out=SD.filled(self.pkg, sst, len(aus), with_ps))


def model(pkg, one, cfg, st, rows, cc, sst=None, hdr=None, with_ps=False, tab=None, host_check=False):
    """The contract of a streams call spelt out with the one-unit forms (`one`: HostOne, or the device calls).  st
    (AAC_STREAM_DT [S]) and sst (sbr_streams rows, None: the AAC call) are left alone.  host_check: every position is
    also held against the host parser (PC.compare, and SD.compare with the header table `tab` for HE).
    Returns dict(records [S * T] ..., status, taken, hold, st, sst, putback = units whose AAC state was put back)."""
    T, S = len(rows), len(rows[0])
    st = st.copy()
    he = sst is not None
    sst = sst.copy() if he else None
    alive = np.ones(S, bool)
    taken = np.zeros(S, np.uint32)
    pos, putback = [], 0
    for t in range(T):
        aus = [rows[t][s] if alive[s] else b"" for s in range(S)]
        st_before = st.copy()
        a = one.aac(cfg, st, aus, cc)
        if host_check:
            PC.compare(pkg, cfg, st_before, aus, cc, a, st)
        status = np.asarray(a["status"]).copy()
        rec = {k: a[k] for k in AAC_KEYS}
        if he:
            b = one.sbr(cfg, sst, aus, a["info"], hdr, status, with_ps)
            if host_check:
                st_h, sst_h = st_before.copy(), sst.copy()
                host = SD.host_parse(pkg, cfg, st_h, sst_h, tab, aus, cc, with_ps)
                SD.compare(pkg, host, sst_h, sst, b)
            only_sbr = (status == 0) & (np.asarray(b["status"]) != 0)
            status = np.asarray(b["status"]).copy()
            sst = b["sst"]
            st[only_sbr] = st_before[only_sbr]                  # the stricter rule of the streams call
            putback += int(only_sbr.sum())
            rec.update(sbr=b["sbr"], ps=b["ps"])
        alive &= status == 0
        taken += alive
        pos.append(rec)
    n = S * T
    out = {}
    for k in pos[0]:
        if pos[0][k] is None:
            out[k] = None
            continue
        first = np.asarray(pos[0][k])
        a = np.zeros((S, T) + first.shape[1:], first.dtype)
        for t in range(T):
            a[:, t] = np.asarray(pos[t][k])
        out[k] = a.reshape((n,) + first.shape[1:])
    hold = (np.arange(T)[None, :] >= taken[:, None]).astype(np.uint8).reshape(n)
    out.update(status=hold.astype(np.int32), taken=taken, hold=hold, st=st, sst=sst, putback=putback)
    return out


def compare_with_model(pkg, got, st_got, mdl, S, T):
    """Everything the contract specifies, byte for byte: status, taken, hold whole; the records of the units taken;
    both final states."""
    n = S * T
    assert np.array_equal(np.asarray(got["taken"]).astype(np.int64), mdl["taken"].astype(np.int64)), (got["taken"], mdl["taken"])
    assert np.array_equal(np.asarray(got["status"]), mdl["status"]), np.flatnonzero(np.asarray(got["status"]) != mdl["status"])[:8]
    assert np.array_equal(np.asarray(got["hold"]), mdl["hold"])
    ok = mdl["status"] == 0
    for k in HE_KEYS:
        if mdl.get(k) is None:
            continue
        a, b = PC.rows(got[k], n)[ok], PC.rows(mdl[k], n)[ok]
        diff = (a != b).any(axis=1)
        assert not diff.any(), (k, np.flatnonzero(ok)[diff][:8], np.flatnonzero(a[diff][0] != b[diff][0])[:8])
    sa, sb = PC.rows(st_got, S), PC.rows(mdl["st"], S)
    assert np.array_equal(sa, sb), ("AAC state", np.flatnonzero((sa != sb).any(axis=1))[:8])
    if mdl["sst"] is not None:
        sa, sb = PC.rows(got["sst"], S), PC.rows(mdl["sst"], S)
        assert np.array_equal(sa, sb), ("SBR state", np.flatnonzero((sa != sb).any(axis=1))[:8])


def host_chain(pkg, cfg, st, rows, cc, sst=None, tab=None, with_ps=False, start=None):
    """The host parser alone over the same units: stream s from position start[s] (default 0) to the end, from st /
    sst (left alone).  Returns dict(records [S * T] -- FILL where a position was not parsed --, status [S * T], st, sst)."""
    T, S = len(rows), len(rows[0])
    n = S * T
    he = sst is not None
    st = st.copy()
    sst = sst.copy() if he else None
    start = np.zeros(S, np.int64) if start is None else np.asarray(start).astype(np.int64)
    out = filled_streams(pkg, S, T, cc, sst if he else None, with_ps)
    out["status"][...] = 0
    keys = [k for k in (HE_KEYS if he else AAC_KEYS) if out.get(k) is not None]
    for t in range(T):
        idx = np.flatnonzero(start <= t)
        if not idx.size:
            continue
        aus = [rows[t][s] for s in idx]
        sub = st[idx].copy()
        if he:
            ssub = sst[idx].copy()
            h = SD.host_parse(pkg, cfg, sub, ssub, tab, aus, cc, with_ps)
            sst[idx] = ssub
        else:
            h = PC.host_parse(pkg, cfg, sub, aus, cc)
        st[idx] = sub
        for k in keys:
            if k in h and h[k] is not None:
                out[k][idx * T + t] = h[k]
        out["status"][idx * T + t] = h["status"]
    out.update(st=st, sst=sst)
    return out


def check_against_host(pkg, cfg, got, st_got, st0, rows, cc, sst0=None, tab=None, with_ps=False):
    """The three rules against the host parser, and the resume:
      OK here            => the all-host chain takes the unit (0, or HEAAC_PARSE_NO_SBR for HE) and writes the same bytes
      the host refuses   => the stream has stopped by then
      a stopped stream   => from the states the call left, the host parser parses units t0 .. T - 1 to what the all-host
                            chain has for them, and ends in the same states
    (an HE unit's AAC records are compared where the host's AAC half took it: SD.host_parse keeps no AAC record)."""
    T, S = len(rows), len(rows[0])
    n = S * T
    he = sst0 is not None
    full = host_chain(pkg, cfg, st0, rows, cc, sst0, tab, with_ps)
    taken = np.asarray(got["taken"]).astype(np.int64)
    ok = (np.arange(T)[None, :] < taken[:, None]).reshape(n)
    takes = np.isin(full["status"], (0, pkg.PARSE_NO_SBR)) if he else full["status"] == 0
    assert not (ok & ~takes).any(), ("OK here, not on the host", np.flatnonzero(ok & ~takes)[:8])
    keys = ("info", "sbr", "ps") if he else AAC_KEYS
    for k in keys:
        if full.get(k) is None:
            continue
        a, b = PC.rows(got[k], n)[ok], PC.rows(full[k], n)[ok]
        diff = (a != b).any(axis=1)
        assert not diff.any(), (k, np.flatnonzero(ok)[diff][:8])
    rest = host_chain(pkg, cfg, st_got, rows, cc, got["sst"] if he else None, tab, with_ps, start=taken)
    for k in keys + ("status",):
        if full.get(k) is None:
            continue
        a, b = PC.rows(rest[k], n)[~ok], PC.rows(full[k], n)[~ok]
        diff = (a != b).any(axis=1)
        assert not diff.any(), ("resumed at t0", k, np.flatnonzero(~ok)[diff][:8])
    assert np.array_equal(PC.rows(rest["st"], S), PC.rows(full["st"], S)), "AAC state after the resumed chain"
    if he:
        assert np.array_equal(PC.rows(rest["sst"], S), PC.rows(full["sst"], S)), "SBR state after the resumed chain"
    return full


# ---- units a stream must stop at ----
AAC_STOPS = ["pulse", "cce", "second_sce", "truncated", "empty", "tag_change"]


def aac_stop_unit(rng, si, aot, cpe, kind, good):
    if kind == "pulse":
        while True:
            au, e = TP._write_au(rng, si, aot, cpe, extras=True)
            if any(d["pulse"] for d in e["ch"]):
                return au
    with PC.no_pulses():
        if kind == "cce":
            cces = [(3, [(1 if cpe else 0, 0, int(rng.integers(0, 4)) if cpe else 2)], 1, True)]
            return TW.build_au(rng, si, aot, cpe, cces, pce=False)[0]
        if kind == "second_sce":
            first = (RU.cpe_element if cpe else RU.sce_element)(rng, si, aot, "good")[0]
            return RU._bytes(first + RU.sce_element(rng, si, aot, "good", tag=1)[0] + RU.END)
        if kind == "tag_change":
            return RU._bytes((RU.cpe_element if cpe else RU.sce_element)(rng, si, aot, "good", tag=5)[0] + RU.END)
    return good[:max(1, len(good) // 2)] if kind == "truncated" else b""


HE_STOPS = ["new_header", "limiter", "misplaced", "bad_grid", "flipped", "aac_refused"]      # classes of SD.mixed_units


def stop_plan(rng, kinds, places, T, whole=3):
    """(kind, t0) per stream: every kind at every place, `whole` streams that do not stop, shuffled so that the
    stopping units of neighbouring streams mostly sit at different positions."""
    plan = [(kind, places[(i + j) % len(places)]) for i, kind in enumerate(kinds) for j in range(len(places))]
    plan = [(k, t0 if k != "tag_change" or t0 else T - 2) for k, t0 in plan]      # the lock needs a unit taken first
    plan += [(None, T)] * whole
    plan = [plan[int(i)] for i in rng.permutation(len(plan))]
    assert sum(a[1] != b[1] for a, b in zip(plan, plan[1:])) >= len(plan) // 2
    return plan
